"""CPU-only checks of the max-IoU anchor assigner (csrc/assign.hip, Calc.assignAnchorsFrames): the rule itself
(tests/assign_ref.assign_from_iou) on the reference arithmetic's f32 IoUs against the float64 truth, against the reference's walk
where the two should agree, on the inputs that show why the rule exists, and on hand-written IoU tables; the C ABI's symbols and
argument checks; the Python and command-line switches.

Measured here (printed by the first test before it asserts): anchors / ground truths that an f32 IoU within IOU_BOUND = 3e-4 of
the truth could decide differently -- 24x20x2: 0.21 % / 1;  16x12x1: 1.04 % / 3;  12x10x3: 0.56 % / 1;  24x20x2 with many_gts: 0 / 0.
The ground truths are the truck (14 anchors lie wholly inside it: 14 equal best IoUs) and, at A = 1, the two boxes at yaw
pi / 2 on the grid's edge, whose two best anchors are mirror images."""
import ctypes

import numpy as np
import pytest

import assign_cases as AC
import assign_ref as AR
import targets_cases as C


def _agree(a, b, n, skip_anchors, skip_gts):
    """Two assign_from_iou results agree on every anchor and ground truth outside the skip masks."""
    pa, ga, na = AR.dense(a, n)
    pb, gb, nb = AR.dense(b, n)
    keep = ~skip_anchors
    assert np.array_equal(pa[keep], pb[keep]), 'positives differ at %s' % np.flatnonzero(keep & (pa != pb))
    assert np.array_equal(ga[keep], gb[keep]), 'matched ground truths differ at %s' % np.flatnonzero(keep & (ga != gb))
    assert np.array_equal(na[keep], nb[keep]), 'not-negatives differ at %s' % np.flatnonzero(keep & (na != nb))
    g_keep = ~skip_gts
    assert np.array_equal(a['c'][g_keep], b['c'][g_keep]) and np.array_equal(a['forced'][g_keep], b['forced'][g_keep])


@pytest.mark.parametrize('name', list(AC.CASES))
def test_rule_on_the_oracle_ious_equals_the_rule_on_the_truth(name):
    c = AC.case(name)
    truth = AC.truth(name)
    iou, stale = AC.oracle_table(name)
    ua, ug = AR.undecidable(truth, AC.NEG, AC.POS, AC.FORCE, C.IOU_BOUND)
    print('%s: %.2f %% of %d anchors and %d of %d ground truths undecidable; largest |oracle - truth| %.2e; %d stale pairs'
          % (name, 100.0 * ua.mean(), c['N'], ug.sum(), len(ug), np.abs(iou - truth).max(), stale.sum()))
    assert ua.mean() <= 0.02 and ug.sum() <= 3
    assert np.abs(iou - truth).max() <= C.IOU_BOUND
    # pairs with stale reads: their anchors and ground truths are left out (the oracle's value there is not the library's)
    skip_a = ua | stale.any(axis=0) | AR.candidates(truth, ug, C.IOU_BOUND)     # ... and which anchor an undecidable box forces
    skip_g = ug | stale.any(axis=1)
    got = AR.assign_from_iou(iou, AC.NEG, AC.POS, AC.FORCE)
    want = AR.assign_from_iou(truth, AC.NEG, AC.POS, AC.FORCE)
    _agree(got, want, c['N'], skip_a, skip_g)
    assert np.abs(got['gt_best'].astype(np.float64) - want['gt_best']).max() <= C.IOU_BOUND
    # what was compared: all but 2 % of the anchors and, per undecidable box, its candidate anchors (at most the 14 inside the truck)
    assert (~skip_a).sum() >= c['N'] - 0.02 * c['N'] - 14 * ug.sum() and (~skip_g).sum() >= 7


def test_thresholds_only_agree_with_the_reference_walk():
    """Car-sized boxes near the axes, no forcing: the positive SET and the not-negative SET are the reference's."""
    name = '24x20x2many'
    c = AC.case(name)
    g = c['g']
    iou, stale = AC.oracle_table(name)
    assert not stale.any()
    ua, _ = AR.undecidable(AC.truth(name), AC.NEG, AC.POS, 2.0, C.IOU_BOUND)
    walk = AC.reference_walk(name)
    pos_ref, neg_ref = np.zeros((c['N'],), bool), np.zeros((c['N'],), bool)
    pos_ref[AC.flat(walk[0], walk[1], walk[2], g)] = True
    neg_ref[AC.flat(walk[3], walk[4], walk[5], g)] = True
    got = AR.assign_from_iou(iou, AC.NEG, AC.POS, 2.0)
    p, _, nn = AR.dense(got, c['N'])
    assert not got['forced'].any() and p.sum() > 40 and nn.sum() > p.sum()
    assert np.array_equal(p[~ua], pos_ref[~ua]) and np.array_equal(nn[~ua], neg_ref[~ua])


def test_the_reason_for_the_feature():
    name = '24x20x2'
    c = AC.case(name)
    g = c['g']
    walk = AC.reference_walk(name)
    walk_flat = AC.flat(walk[0], walk[1], walk[2], g)
    assert np.bincount(walk[6], minlength=10).tolist() == [2, 2, 2, 2, 5, 7, 7, 0, 0, 0]       # +-pi/4 and the truck: nothing
    assert len(walk_flat) == 27 and len(set(walk_flat.tolist())) == 20                          # 7 anchors listed twice
    iou, stale = AC.oracle_table(name)
    assert not stale.any()
    got = AR.assign_from_iou(iou, AC.NEG, AC.POS, AC.FORCE)
    assert len(set(got['pos'].tolist())) == len(got['pos']) and len(set(got['notneg'].tolist())) == len(got['notneg'])
    assert np.all(np.diff(got['pos']) > 0) and np.all(np.diff(got['notneg']) > 0)
    assert set(got['pos'].tolist()) <= set(got['notneg'].tolist())
    # boxes 5 and 6 are the same box: every shared anchor goes to 5, and 6's best anchor is 5's with an equal claim -- so the
    # duplicate is the one box without a positive; every other box has one
    assert got['c'][5] == got['c'][6] and iou[5, got['c'][5]] == iou[6, got['c'][6]] > 0.999
    assert np.bincount(got['gi'], minlength=10).tolist() == [2, 2, 2, 2, 5, 7, 0, 1, 1, 1]
    assert got['forced'].tolist() == [True] * 6 + [False] + [True] * 3
    assert got['pos'].tolist() == [0, 37, 39, 40, 252, 292, 330, 332, 334, 372, 376, 412, 458, 460, 498, 500, 538, 620, 738, 880, 920,
                                   957, 959]
    assert got['gi'].tolist() == [0, 1, 1, 0, 5, 5, 5, 5, 5, 5, 8, 5, 4, 4, 4, 4, 4, 7, 9, 2, 2, 3, 3]
    assert len(got['notneg']) == 49 and got['c'].tolist() == [0, 39, 920, 959, 498, 332, 332, 620, 376, 738]
    # thresholds only: the three boxes the walk leaves out stay out, and the duplicate's share goes to box 5
    thr = AR.assign_from_iou(iou, AC.NEG, AC.POS, 2.0)
    assert np.bincount(thr['gi'], minlength=10).tolist() == [2, 2, 2, 2, 5, 7, 0, 0, 0, 0]
    assert set(thr['pos'].tolist()) == set(walk_flat.tolist())


def _rule(table, neg=0.45, pos=0.6, force=0.1):
    r = AR.assign_from_iou(np.array(table, np.float32), neg, pos, force)
    return r['pos'].tolist(), r['gi'].tolist(), r['notneg'].tolist()


def test_constructed_rule_cases():
    # a tie of two boxes on one anchor: the lowest g
    assert _rule([[0.0, 0.7, 0.0], [0.0, 0.7, 0.0]]) == ([1], [0], [1])
    # a tie of two anchors for one box below the threshold: the lowest anchor is forced, the other is only not negative
    assert _rule([[0.5, 0.0, 0.5]]) == ([0], [0], [0, 2])
    # two boxes forcing one anchor: the larger IoU wins, the other box has no positive; equal IoUs: the lowest g
    assert _rule([[0.0, 0.30, 0.0], [0.0, 0.35, 0.0]]) == ([1], [1], [1])
    assert _rule([[0.0, 0.30, 0.0], [0.0, 0.30, 0.0]]) == ([1], [0], [1])
    # a forced match overrides a threshold match: anchor 0 is box 0's by threshold (0.7; its best is anchor 1) and box 1's best (0.3)
    assert _rule([[0.7, 0.8, 0.0], [0.3, 0.0, 0.0]]) == ([0, 1], [1, 0], [0, 1])
    # ... but not a better forced claim: here anchor 0 is box 0's best as well
    assert _rule([[0.7, 0.65, 0.0], [0.3, 0.0, 0.0]]) == ([0, 1], [0, 0], [0, 1])
    # ... and with force > 1.5 there is none: thresholds only
    assert _rule([[0.7, 0.8, 0.0], [0.3, 0.0, 0.0]], force=2.0) == ([0, 1], [0, 0], [0, 1])
    assert _rule([[0.5, 0.0, 0.5]], force=2.0) == ([], [], [0, 2])
    # a best IoU below force: no positive; at force exactly: forced
    assert _rule([[0.05, 0.0, 0.0]]) == ([], [], [])
    assert _rule([[np.float32(0.1), 0.0, 0.0]]) == ([0], [0], [0])
    # a forced positive below neg is listed as not negative as well
    assert _rule([[0.2, 0.0, 0.5]], neg=0.45)[2] == [2]
    assert _rule([[0.2, 0.0, 0.3]], neg=0.45) == ([2], [0], [2])
    # a frame with no box
    r = AR.assign_from_iou(np.zeros((0, 5), np.float32), 0.45, 0.6, 0.1)
    assert r['pos'].size == 0 and r['gi'].size == 0 and r['notneg'].size == 0 and r['gt_best'].size == 0


def test_assign_symbols_signatures_and_abi_version():
    from modules import Extension as X
    assert X.ABI_VERSION == 10 and X.lib.mvx_abi_version() == 10
    lib = ctypes.CDLL(X.LIB_PATH)
    for name in ('mvx_assign_anchors_frames_workspace_bytes', 'mvx_assign_anchors_frames'):
        assert hasattr(lib, name) and name in X.PROTOTYPES
    res, args = X.PROTOTYPES['mvx_assign_anchors_frames']
    assert res is ctypes.c_int32 and len(args) == 21
    assert args[7:10] == [ctypes.c_float] * 3 and args[10] is ctypes.c_int32 and args[14] is ctypes.c_int64
    res, args = X.PROTOTYPES['mvx_assign_anchors_frames_workspace_bytes']
    assert res is ctypes.c_size_t and args == [ctypes.c_int32] * 5
    q = X.lib.mvx_assign_anchors_frames_workspace_bytes
    one, four = q(15, 1, 176, 200, 2), q(60, 4, 176, 200, 2)
    assert one >= 176 * 200 * 2 * 8 and four > 3 * one             # the key map of every frame at least
    assert q(0, 1, 176, 200, 2) <= 256


def _call(**over):
    """mvx_assign_anchors_frames with plausible arguments (fake, never dereferenced device addresses: every case here must be
    refused by the host-side checks before anything is launched)."""
    from modules import Extension as X
    fake = ctypes.c_void_p(1 << 20)
    a = dict(off=[0, 3], F=1, l=24, w=20, A=2, neg=0.45, pos=0.6, force=0.1, R=5, cap=100, ws_bytes=1 << 40)
    a.update(over)
    off = (ctypes.c_int32 * len(a['off']))(*a['off'])
    return X.lib.mvx_assign_anchors_frames(fake, off, a['F'], fake, a['l'], a['w'], a['A'], a['neg'], a['pos'], a['force'], a['R'], fake,
                                           fake, fake, a['cap'], fake, fake, fake, fake, a['ws_bytes'], None)


@pytest.mark.parametrize('over', [dict(neg=0.7), dict(neg=0.0), dict(neg=-0.1), dict(force=0.0), dict(force=-1.0), dict(R=0), dict(R=56),
                                  dict(F=0), dict(F=17, off=[0] * 18), dict(off=[1, 3]), dict(off=[0, 3, 2], F=2), dict(l=0), dict(A=0),
                                  dict(cap=-1), dict(ws_bytes=16)])
def test_assign_argument_checks(over):
    assert _call(**over) < 0                                       # MVX_EINVAL: refused before anything is launched


def test_calc_rejects_bad_thresholds():
    import torch
    from modules import Calc
    frames = [(torch.zeros((1, 4, 2)), None)]
    anchors = torch.zeros((2, 2, 2, 4, 2))
    with pytest.raises(ValueError):
        Calc.assignAnchorsFrames(frames, anchors, negThr=0.7, posThr=0.6)
    with pytest.raises(ValueError):
        Calc.assignAnchorsFrames(frames, anchors, forceThr=0.0)
    with pytest.raises(ValueError):
        Calc.assignAnchorsFrames(frames, anchors, forceThr=-0.5)
    with pytest.raises(ValueError):
        Calc.assignAnchors(frames[0][0], anchors, negThr=0.0)
    # frames without boxes need no device
    info = {}
    assert Calc.assignAnchorsFrames([None, (torch.zeros((0, 4, 2)), None)], anchors, info=info) == [None, None]
    assert info == dict(gt_best=[None, None], forced_only=0, none=0)


def test_train_like_targets_switch():
    import train_like as T
    a = T.parse_args(['root', '--targets', 'maxiou', '--force-iou', '0.2'])
    assert a.targets == 'maxiou' and a.force_iou == 0.2
    d = T.parse_args(['root'])
    assert d.targets == 'reference' and d.force_iou == 0.1
    assert T.parse_args(['root', '--mode', 'fast', '--loss', 'focal', '--targets', 'maxiou', '--force-iou', '2']).force_iou == 2.0
    with pytest.raises(SystemExit):
        T.parse_args(['root', '--targets', 'best'])
    with pytest.raises(SystemExit):
        T.parse_args(['root', '--force-iou', '0'])


def test_loaders_take_an_assigner():
    import inspect
    from modules import pipeline
    from modules.data import Prefetch
    assert inspect.signature(pipeline.batch_from_dataset).parameters['assigner'].default is None
    assert inspect.signature(Prefetch.PrefetchLoader.__init__).parameters['assigner'].default is None
