"""CPU checks of the direct detection cases (tests/detect_cases.py): every case reaches the path it names.  A numpy mirror of
order_key (detect_cases.order_key) is used for these claims only; the expected results of tests/test_detect_direct_gpu.py come
from tests/detect_ref.py.  Also: detect_ref.greedy_nms_near against detect_ref.greedy_nms."""
import time

import numpy as np
import pytest

import detect_cases as C
import detect_ref as R
import iou_head_ref as IR
import mvx_oracle as O


def _sigmoid64(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _all_cases():
    out = list(C.selection_cases()) + list(C.odd_logit_cases()) + [C.sixteen_frames(), C.decode_case(), C.nonfinite_case(),
                                                                  C.exact_threshold_case()]
    out += [C.word_edge_case(n) for n in C.WORD_EDGE_SIZES] + list(C.scan_cases()) + [C.post_max_case(p) for p in C.POST_MAX]
    return out


def test_no_logit_sits_at_the_score_threshold_and_counts_are_as_stated():
    """Selection must not hinge on the last bit of expf: every sigmoid is 1e-6 away from score_thr (0 admits everything but
    a NaN).  Where a case states its candidate counts, they are the reference's."""
    for case in _all_cases() + [C.full_case()]:
        lg = case['cls']
        p = _sigmoid64(lg[~np.isnan(lg)])
        if case['score_thr'] > 0:
            assert (np.abs(p - case['score_thr']) > 1e-6).all(), case['name']
        if 'counts' in case:
            got = [R.candidates(lg[f], case['score_thr'], case['pre_max'])[1] for f in range(case['F'])]
            assert got == list(case['counts']), (case['name'], got)


def _cut_keys(keys, K):
    s = np.sort(keys.astype(np.int64))[::-1]
    return int(s[K - 1]), int(s[K])


@pytest.mark.parametrize('name', ['last_digit', 'third_digit', 'kth_negative', 'rectified'])
def test_the_stated_digit_decides_the_cut(name):
    case = C.rectified_case() if name == 'rectified' else {c['name']: c for c in C.selection_cases()}[name]
    K = case['pre_max']
    for f in range(case['F']):
        lg = case['cls'][f]
        cand = _sigmoid64(lg) >= case['score_thr']
        assert cand.sum() > K
        keys = C.order_key(lg[cand])
        kth, nxt = _cut_keys(keys, K)
        prefix, byte = case['cut'][f]
        sh = 8 * (byte + 1)
        assert kth > nxt and kth >> sh << sh == prefix and nxt >> sh << sh == prefix, (name, f, hex(kth), hex(nxt))
        assert (kth >> 8 * byte) & 255 != (nxt >> 8 * byte) & 255
        digits = [len(set(((keys.astype(np.int64) >> 8 * b) & 255).tolist())) for b in range(4)]
        print('%s frame %d: %d candidates, K-th key %08x, next %08x, byte %d decides, distinct digits per byte %s'
              % (name, f, cand.sum(), kth, nxt, byte, digits))
        assert digits[0] > 100 and (name in ('last_digit', 'rectified') or digits[1] > 50)
        if name == 'kth_negative':
            assert C.key_to_float([kth])[0] < 0 and (keys.astype(np.int64) > kth).sum() > K // 3      # the cut is among the negatives
    assert len({b for _, b in case['cut']}) == (2 if name == 'kth_negative' else 1)


def test_ties_at_the_cut_span_three_compaction_chunks():
    case = {c['name']: c for c in C.selection_cases()}['ties_at_cut']
    K = case['pre_max']
    needs = []
    for f, t in enumerate(case['ties']):
        keys = C.order_key(case['cls'][f]).astype(np.int64)
        cand = _sigmoid64(case['cls'][f]) >= case['score_thr']
        kth, _ = _cut_keys(keys[cand], K)
        tied = np.nonzero(cand & (keys == kth))[0]
        above = int((cand & (keys > kth)).sum())
        print('ties_at_cut frame %d: m = %d, need = %d, chunks of the ties %s' % (f, t['m'], t['need'], t['chunks']))
        assert np.array_equal(tied, t['tied']) and len(tied) == t['m'] and K - above == t['need'] and cand.sum() > K
        assert len(t['chunks']) >= 3 and t['chunks'] == sorted(set((tied // C.CHUNK).tolist()))
        taken = tied[:t['need']]
        assert len(set((taken // C.CHUNK).tolist())) >= (3 if t['need'] >= 200 else 1)     # there the taken ties cross chunks too
        ref = R.candidates(case['cls'][f], case['score_thr'], K)[0]
        assert np.array_equal(np.sort(ref[above:]), taken)
        needs.append((t['need'], t['m']))
    assert needs[0][1] > 5 * needs[0][0] and needs[1][0] == 1 and needs[2][0] == needs[2][1] and needs[3] == (200, 300)


def test_sort_sizes():
    seen = {}
    for case in C.selection_cases():
        if not case['name'].startswith('sort_'):
            continue
        for f in range(case['F']):
            n_sel = min(R.candidates(case['cls'][f], case['score_thr'], case['pre_max'])[1], case['pre_max'])
            assert n_sel == case['n_sel'] and C.sort_size(n_sel) == case['P']
        seen[case['n_sel']] = case['P']
        print('%s: n_sel %d, P %d, %d padding zeros' % (case['name'], case['n_sel'], case['P'], case['P'] - case['n_sel']))
    assert seen == {1000: 1024, 1024: 1024, 1025: 2048, 2048: 2048, 2049: 4096, 4096: 4096}


def test_rectified_scores_are_apart():
    """No two distinct rectified scores can round to the same float: the float64 log scores s (what is keyed) and the scores
    exp(s) of the candidates are either equal or more than 1e-5 apart, relatively."""
    case = C.rectified_case()
    for f in range(case['F']):
        s = IR.rectified_log(case['cls'][f], case['iou'][f], case['alpha'])
        s = np.unique(s[np.exp(s) >= case['score_thr']])
        for v in (s, np.exp(s)):
            gap = np.abs(np.diff(v)) / np.abs(v[1:])
            print('rectified frame %d: %d distinct values, minimum relative gap %.3g' % (f, len(v), gap.min()))
            assert gap.min() > 1e-5
        keep, _, n = IR.candidates(case['cls'][f], case['iou'][f], case['alpha'], case['score_thr'], case['pre_max'])
        assert n > case['pre_max'] and np.array_equal(keep, R.candidates(case['cls'][f], case['score_thr'], case['pre_max'])[0])


# ---- mask and scan --------------------------------------------------------------------------------------------------------
def _rank_boxes(case, f):
    mine = case['rank_anchor'][f]
    with np.errstate(over='ignore'):
        return R.decode(case['reg'][f, mine], case['anchors'][mine], 'loss')


def _iou64(qa, qb):
    inter = IR.clip_area(qa, qb)
    return inter / (abs(IR._area(qa)) + abs(IR._area(qb)) - inter)


def _placed_cases():
    return ([C.word_edge_case(n) for n in C.WORD_EDGE_SIZES] + list(C.scan_cases()) + [C.post_max_case(p) for p in C.POST_MAX]
            + [C.nonfinite_case(), C.exact_threshold_case()])


@pytest.mark.parametrize('case', _placed_cases(), ids=lambda c: c['name'])
def test_placed_boxes_overlap_as_intended_and_nowhere_else(case):
    """In float64: every intended overlap has IoU above 0.5, every other pair has its bounding circles apart (IoU exactly 0).
    Two exceptions, both stated by their cases: the chain 0 - 10 - 70 of 'suppressed_suppressor' has IoU 0.44 per link (above
    0.5 the two ends would have to intersect), and 'exact_threshold' holds one pair at exactly iou_thr.  The stated kept ranks
    are what greedy NMS over exactly these overlaps keeps, and what detect_ref.greedy_nms keeps on the reference corners."""
    for f in range(case['F']):
        boxes = _rank_boxes(case, f)
        n = case['n_ranks'][f]
        bad = set(case.get('bad', [[]] * case['F'])[f])
        fin = [r for r in range(n) if r not in bad]
        with np.errstate(over='ignore'):
            finite = np.isfinite(boxes.astype(np.float32)).all(1)      # exp(200) overflows in f32, the device's format
        assert finite[fin].all() and not finite[sorted(bad)].any()
        quads = np.stack([IR.quad64(boxes[r]) if r not in bad else np.zeros((4, 2)) for r in range(n)])
        cen = quads.mean(1)
        rad = np.sqrt(((quads - cen[:, None]) ** 2).sum(2)).max(1)
        gap = np.sqrt(((cen[:, None] - cen[None]) ** 2).sum(2)) - (1.01 * (rad[:, None] + rad[None]) + 1e-3)
        want = set()
        for grp in case['groups'][f]:
            want |= {(a, b) for a in grp for b in grp if a < b and a not in bad and b not in bad}
        floor = {}
        if f == 0:
            for a, b in case.get('chain', ()):
                want.add((a, b))
                floor[(a, b)] = 0.4
        if 'exact' in case:
            a, b, val = case['exact'][f]
            want.add((a, b))
            floor[(a, b)] = val - 1e-12
            corners = R.corners(boxes[[a, b]])
            assert O.bbox_pairwise(corners[:1], corners[1:], True)[0, 0] == np.float32(val)      # exact in the f32 clipping too
            assert val in (case['iou_thr'], 0.3125)
        ious = {(a, b): _iou64(quads[a], quads[b]) for a, b in want}
        for a, b in want:
            assert ious[(a, b)] > floor.get((a, b), 0.5), (case['name'], f, a, b)
        for a in fin:
            for b in fin:
                if a < b and (a, b) not in want:
                    assert gap[a, b] > 0, (case['name'], f, a, b)
        removed, keep = set(), []
        for r in fin:
            if r in removed:
                continue
            keep.append(r)
            removed |= {b for a, b in want if a == r and ious[(a, b)] > case['iou_thr'] + 1e-9}
        assert keep == case['keep'][f], (case['name'], f)
        ref = R.greedy_nms(R.corners(boxes[fin]), case['iou_thr'], n)
        assert [fin[k] for k in ref] == keep
        assert np.array_equal(R.candidates(case['cls'][f], case['score_thr'], case['pre_max'])[0], case['rank_anchor'][f])


def test_word_edge_cases_hit_the_bits_they_name():
    for n in C.WORD_EDGE_SIZES:
        case = C.word_edge_case(n)
        assert case['n_ranks'] == [n] * 3
        if n >= 65:
            assert (63, 64) in case['groups'][1] and 64 not in case['keep'][1] and 63 in case['keep'][1]
        if n >= 66:
            assert 65 not in case['keep'][1] and 0 in case['keep'][1]
        if n >= 64:
            assert (62, 63) in case['groups'][2] and 63 not in case['keep'][2]
        if n > 66:
            assert n - 1 in case['groups'][0][0] and case['keep'][0][:3] == [0, 2, 3]
    chunk = C.scan_cases()[0]
    assert chunk['keep'][0] == list(range(64)) + list(range(128, 141))
    assert 70 in C.scan_cases()[1]['keep'][0] and 10 not in C.scan_cases()[1]['keep'][0]
    assert C.nonfinite_case()['rank_anchor'][0][200] >= 0 and 200 // 64 == 3


# ---- full size --------------------------------------------------------------------------------------------------------------
def test_near_reference_equals_the_full_table():
    quads = C.near_check_case()
    assert quads.shape == (600, 4, 2)
    for thr, post in ((0.1, 600), (0.01, 600), (0.5, 600), (0.1, 50)):
        a, b = R.greedy_nms(quads, thr, post), R.greedy_nms_near(quads, thr, post)
        assert a == b and 50 <= len(a) <= 600
    assert R.greedy_nms_near(quads[:0], 0.1, 5) == [] and R.greedy_nms_near(quads[:1], 0.1, 5) == [0]


def test_full_case_has_no_pair_at_the_threshold_and_crosses_words():
    """Over all 4224 boxes: no pair's oracle IoU on the reference corners within 1e-3 of iou_thr.  Per frame, in candidate order:
    at least 300 kept, and a kept candidate of word 0 suppresses one of a word >= 32."""
    case = C.full_case()
    quads = R.corners(case['anchors'])
    for cols, iou in zip(*R.near_pairs(quads)):
        assert not (np.abs(iou - case['iou_thr']) < C.BAND).any()
    for f in range(case['F']):
        idx = R.candidates(case['cls'][f], case['score_thr'], case['pre_max'])[0]
        assert len(idx) == 4096
        t0 = time.perf_counter()
        pairs = R.near_pairs(quads[idx])
        keep = R.greedy_nms_near(quads[idx], case['iou_thr'], 4096, pairs)
        dt = time.perf_counter() - t0
        removed = np.zeros(4096, bool)
        far = 0
        for i in keep:
            hit = pairs[0][i][(pairs[1][i] > case['iou_thr']) & (pairs[0][i] > i)]
            if i < 64:
                far += int((~removed[hit] & (hit >= 32 * 64)).sum())
            removed[hit] = True
        print('full frame %d: %d kept of 4096, %d suppressions from word 0 into words >= 32, reference %.2f s' % (f, len(keep), far, dt))
        assert len(keep) >= 300 and far >= 1
