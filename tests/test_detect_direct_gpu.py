"""The four detection kernels (csrc/detect.hip: detect_keys, detect_select, detect_mask, detect_scan) called directly through
_hip.detect_frames on the small hand-made cases of tests/detect_cases.py: the radix select's digits and rank bookkeeping, the
ordered compaction's ties and chunks, every size of the bitonic sort, the mask's word edges, the scan's chunks, post_max and
non-finite lanes, odd logits, and the workspace.  Indices, counts, status bits and boxes are compared exactly with
tests/detect_ref.py; the only tolerances are the decode's 1e-6 of decode_scale and the score's rtol 1e-6, both taken over from
tests/test_detect_gpu.py.  tests/test_detect_direct_host.py checks on the CPU that every case reaches the path it names.

Which tests notice which fault (each tried once on a scratch build of csrc/detect.hip / bev_iou.h, MI355X):
  * sort key low word ``index`` in place of ``~index`` (read back without the ``~``): test_selection_and_order[last_digit,
    third_digit, kth_negative, ties_at_cut], test_rectified_score_order, test_odd_logits,
    test_sixteen_frames_equal_their_single_runs, test_scan_chunks[identical];
  * order_key without the ``x == 0.f`` fold: test_odd_logits;
  * detect_scan without ``word |= s_rows[r][cw]``: test_mask_word_edges[2 .. 129], test_scan_chunks[suppressed_suppressor,
    identical], test_nonfinite_candidate_in_a_later_lane, test_iou_exactly_at_the_threshold,
    test_full_size_matches_the_near_reference, test_stale_workspace_bits_are_never_read;
  * detect_scan with ``lane == 0`` for ``lane < nw`` on the ``rem |=`` line: test_mask_word_edges[65, 128, 129],
    test_scan_chunks[chunk_removed, identical], test_full_size_matches_the_near_reference,
    test_stale_workspace_bits_are_never_read;
  * detect_mask with ``j < i`` for ``j <= i`` and ``iou >= iou_thr`` for ``>``: test_iou_exactly_at_the_threshold alone (the
    diagonal bit is never consulted; only a pair at exactly iou_thr tells the two comparisons apart)."""
import functools

import numpy as np
import pytest
import torch

import detect_cases as C
import detect_ref as R
import iou_head_ref as IR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
TRUNCATED, NONFINITE = 1, 2
LAYOUTS = ('rows', 'nchw', 'strided')


def _heads(case, layout, frames):
    """(cls (F,l,w,A), reg (F,l,w,7A), iou or None) device views of the case's frames: 'rows' = channels-last rows
    (F*l*w, 8A [+ A]) sliced; 'nchw' = maps permuted; 'strided' = rows inside a larger NaN-filled buffer, 3 rows between the
    frames and a column on either side."""
    F, l, w, A = len(frames), case['l'], case['w'], case['A']
    cls = torch.from_numpy(case['cls'][frames]).view(F, l, w, A)
    reg = torch.from_numpy(case['reg'][frames]).view(F, l, w, 7 * A)
    parts = [cls, reg] + ([torch.from_numpy(case['iou'][frames]).view(F, l, w, A)] if 'iou' in case else [])
    if layout == 'nchw':
        out = [p.permute(0, 3, 1, 2).contiguous().to(DEV).permute(0, 2, 3, 1) for p in parts]
    else:
        rows = torch.cat(parts, 3).view(F, l * w, -1)
        if layout == 'strided':
            buf = torch.full((F, l * w + 3, rows.shape[2] + 2), float('nan'))
            buf[:, :l * w, 1:-1] = rows
            v = buf.to(DEV)[:, :l * w, 1:-1].unflatten(1, (l, w))
            assert F == 1 or v.stride(0) != l * w * v.stride(2)
        else:
            v = rows.contiguous().to(DEV).view(F, l, w, -1)
        out = [v[..., :A], v[..., A:8 * A]] + ([v[..., 8 * A:9 * A]] if 'iou' in case else [])
    return out[0], out[1], (out[2] if 'iou' in case else None)


def run(case, layout='rows', frames=None, **over):
    """_hip.detect_frames(debug=True) on the case -> dict of host numpy arrays (boxes, scores, idx, meta, cand_idx, cand_boxes,
    cand_corners)."""
    from modules import _hip
    frames = list(range(case['F'])) if frames is None else list(frames)
    cls, reg, iou = _heads(case, layout, frames)
    kw = dict(score_thr=case['score_thr'], iou_thr=case['iou_thr'], pre_max=case['pre_max'], post_max=case['post_max'],
              decode=case['decode'])
    kw.update(over)
    anchors = torch.from_numpy(case['anchors']).to(DEV).view(case['l'], case['w'], case['A'], 7)
    res = _hip.detect_frames(cls, reg, anchors, len(frames), case['l'], case['w'], case['A'], kw['score_thr'], kw['iou_thr'],
                             kw['pre_max'], kw['post_max'], kw['decode'], debug=True, iou_logits=iou, iou_alpha=case.get('alpha', 0.5))
    torch.cuda.synchronize()
    names = ('boxes', 'scores', 'idx', 'meta', 'cand_idx', 'cand_boxes', 'cand_corners')
    return {k: v.cpu().numpy() for k, v in zip(names, res)}


def same(a, b):
    """Bitwise equality (floats by their bit patterns: a NaN equals itself, -0 differs from +0)."""
    a, b = (v.view(np.uint32) if v.dtype == np.float32 else v for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


def expected_candidates(case, f):
    if 'iou' in case:
        keep, _, n = IR.candidates(case['cls'][f], case['iou'][f], case['alpha'], case['score_thr'], case['pre_max'])
        return keep, n
    return R.candidates(case['cls'][f], case['score_thr'], case['pre_max'])


def check_selection(case, out, frames=None):
    """cand_idx, n_candidates and TRUNCATED exactly; returns the reference's candidate lists."""
    frames = list(range(case['F'])) if frames is None else frames
    K = case['pre_max']
    refs = []
    for o, f in enumerate(frames):
        ref_idx, n_above = expected_candidates(case, f)
        n = len(ref_idx)
        assert out['meta'][1, o] == n_above, (case['name'], f, out['meta'][1, o], n_above)
        assert out['meta'][2, o] & TRUNCATED == (TRUNCATED if n_above > K else 0), (case['name'], f)
        got = out['cand_idx'][o]
        assert np.array_equal(got[:n], ref_idx), (case['name'], f, np.nonzero(got[:n] != ref_idx)[0][:8])
        assert (got[n:] == -1).all(), (case['name'], f)
        refs.append(ref_idx)
    return refs


def check_disjoint_outputs(case, out, refs):
    """Zero regression and boxes that cannot touch: the candidates' boxes are their anchors bit for bit, the first post_max
    candidates are the output, the rows after them are zero with index -1."""
    P = out['idx'].shape[1]
    for o, ref_idx in enumerate(refs):
        n = len(ref_idx)
        assert np.array_equal(out['cand_boxes'][o, :n].view(np.uint32), case['anchors'][ref_idx].view(np.uint32)), (case['name'], o)
        k = min(n, P)
        assert out['meta'][0, o] == k and out['meta'][2, o] & NONFINITE == 0
        assert np.array_equal(out['idx'][o, :k], ref_idx[:k]) and (out['idx'][o, k:] == -1).all()
        assert np.array_equal(out['boxes'][o, :k].view(np.uint32), case['anchors'][ref_idx[:k]].view(np.uint32))
        assert not out['boxes'][o, k:].any() and not out['scores'][o, k:].any()


def check_nms(case, out, refs, near=False):
    """Kept indices, counts, boxes and scores exactly against greedy NMS on the device's own corners (the non-finite
    candidates left out, as they start removed)."""
    P = out['idx'].shape[1]
    for o, ref_idx in enumerate(refs):
        n = len(ref_idx)
        ok = np.isfinite(out['cand_boxes'][o, :n]).all(1)
        pos = np.nonzero(ok)[0]
        quads = np.ascontiguousarray(out['cand_corners'][o, pos], np.float32)
        keep = (R.greedy_nms_near if near else R.greedy_nms)(quads, case['iou_thr'], P)
        keep = pos[keep] if len(keep) else np.zeros(0, np.int64)
        k = len(keep)
        assert out['meta'][0, o] == k, (case['name'], o, out['meta'][0, o], k)
        assert (out['meta'][2, o] & NONFINITE != 0) == (not ok.all())
        assert np.array_equal(out['idx'][o, :k], ref_idx[keep]), (case['name'], o)
        assert (out['idx'][o, k:] == -1).all() and not out['boxes'][o, k:].any() and not out['scores'][o, k:].any()
        assert np.array_equal(out['boxes'][o, :k].view(np.uint32), out['cand_boxes'][o, keep].view(np.uint32))
        if 'iou' not in case:
            want = torch.sigmoid(torch.from_numpy(case['cls'][o][ref_idx[keep]]))
            assert torch.allclose(torch.from_numpy(out['scores'][o, :k]), want, rtol=1e-6, atol=0)


# ---- selection and order ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(C.selection_cases())), ids=[c['name'] for c in C.selection_cases()])
def test_selection_and_order(k):
    case = C.selection_cases()[k]
    layout = LAYOUTS[k % 3]
    out = run(case, layout)
    refs = check_selection(case, out)
    check_disjoint_outputs(case, out, refs)
    if 'counts' in case:
        assert out['meta'][1].tolist() == list(case['counts'])
    if case['score_thr'] == 0.0:
        assert (out['meta'][1] == case['N']).all()                     # the tail slots of npad are no candidates


def test_rectified_score_order():
    case = C.rectified_case()
    out = run(case, 'nchw')
    refs = check_selection(case, out)
    check_disjoint_outputs(case, out, refs)
    for f, ref_idx in enumerate(refs):
        want = IR.candidates(case['cls'][f], case['iou'][f], case['alpha'], case['score_thr'], case['pre_max'])[1]
        np.testing.assert_allclose(out['scores'][f, :len(ref_idx)], want, rtol=1e-5, atol=0)      # tests/test_iou_head_gpu.py's bound


def test_odd_logits():
    """NaN never a candidate; +inf first with score exactly 1; -inf at score_thr 0 the last candidate with score exactly 0 and no
    candidate at 0.05; -0.0 and +0.0 tie, the lower anchor index first whichever it holds."""
    for case, layout in zip(C.odd_logit_cases(), LAYOUTS):
        out = run(case, layout)
        refs = check_selection(case, out)
        check_disjoint_outputs(case, out, refs)
        for f in range(2):
            got = out['cand_idx'][f]
            n = int((got >= 0).sum())
            assert not set(got[:n].tolist()) & {2, 17, 44}
            assert got[0] == 30 and out['scores'][f, 0] == 1.0
            at5, at9 = int(np.nonzero(got == 5)[0][0]), int(np.nonzero(got == 9)[0][0])
            assert at9 == at5 + 1, (case['name'], f, at5, at9)
            if case['name'] == 'odd_thr0':
                assert got[n - 1] == 12 and out['scores'][f, n - 1] == 0.0 and n == 42
            if case['score_thr'] > 0:
                assert 12 not in got[:n].tolist() and n == 41
            k = out['meta'][0, f]
            fin = np.isfinite(case['cls'][f][got[:k]])
            want = torch.sigmoid(torch.from_numpy(case['cls'][f][got[:k]][fin]))
            assert torch.allclose(torch.from_numpy(out['scores'][f, :k][fin]), want, rtol=1e-6, atol=0)


def test_sixteen_frames_equal_their_single_runs():
    case = C.sixteen_frames()
    assert case['F'] == 16
    out = run(case, 'rows')
    check_disjoint_outputs(case, out, check_selection(case, out))
    assert (out['meta'][1] == 0).sum() == 3
    for f in range(16):
        one = run(case, 'rows', frames=[f])
        for k in out:
            a, b = (out[k][:, f], one[k][:, 0]) if k == 'meta' else (out[k][f], one[k][0])
            if k in ('cand_boxes', 'cand_corners'):                    # rows past n_sel are not written
                n = int((out['cand_idx'][f] >= 0).sum())
                a, b = a[:n], b[:n]
            assert same(a, b), (f, k)


# ---- decode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['loss', 'reference'])
def test_decode_three_anchors_per_cell(mode):
    case = C.decode_case()
    out = run(case, 'nchw' if mode == 'loss' else 'strided', decode=mode)
    refs = check_selection(case, out)
    for f, ref_idx in enumerate(refs):
        assert len(ref_idx) == 45
        reg, anc = case['reg'][f, ref_idx], case['anchors'][ref_idx]
        err = np.abs(out['cand_boxes'][f, :45].astype(np.float64) - R.decode(reg, anc, mode)) / R.decode_scale(reg, anc, mode)
        assert err.max() <= 1e-6, (mode, f, err.max())
        want_c = R.corners(out['cand_boxes'][f, :45])
        assert np.all(np.abs(out['cand_corners'][f, :45] - want_c) <= 1e-5 * np.maximum(np.abs(want_c), 1.0))
        k = out['meta'][0, f]
        assert 0 < k <= 45 and out['meta'][2, f] == 0
        at = [ref_idx.tolist().index(i) for i in out['idx'][f, :k]]
        assert at == sorted(at) and at[0] == 0
        assert np.array_equal(out['boxes'][f, :k].view(np.uint32), out['cand_boxes'][f, at].view(np.uint32))
        want_s = torch.sigmoid(torch.from_numpy(case['cls'][f][out['idx'][f, :k]]))
        assert torch.allclose(torch.from_numpy(out['scores'][f, :k]), want_s, rtol=1e-6, atol=0)


@pytest.mark.parametrize('mode', ['loss', 'reference'])
def test_zero_regression_returns_the_anchors_bitwise(mode):
    case = dict(C.decode_case())
    case['reg'] = np.zeros_like(case['reg'])
    out = run(case, 'rows', decode=mode)
    for f, ref_idx in enumerate(check_selection(case, out)):
        assert np.array_equal(out['cand_boxes'][f, :45].view(np.uint32), case['anchors'][ref_idx].view(np.uint32))


# ---- mask and scan --------------------------------------------------------------------------------------------------------
def check_placed(case, out):
    """The reference on the device's corners, and the ranks the case itself says are kept."""
    refs = check_selection(case, out)
    check_nms(case, out, refs)
    P = out['idx'].shape[1]
    for f in range(case['F']):
        assert np.array_equal(refs[f], case['rank_anchor'][f])
        keep = case['keep'][f][:P]
        assert out['meta'][0, f] == len(keep) and np.array_equal(out['idx'][f, :len(keep)], case['rank_anchor'][f][keep]), (case['name'], f)


@pytest.mark.parametrize('n', C.WORD_EDGE_SIZES)
def test_mask_word_edges(n):
    case = C.word_edge_case(n)
    out = run(case, LAYOUTS[n % 3])
    assert (out['meta'][1] == n).all()
    check_placed(case, out)


@pytest.mark.parametrize('k', range(len(C.scan_cases())), ids=[c['name'] for c in C.scan_cases()])
def test_scan_chunks(k):
    case = C.scan_cases()[k]
    check_placed(case, run(case, LAYOUTS[k % 3]))


@pytest.mark.parametrize('post_max', C.POST_MAX)
def test_post_max_in_mid_chunk_and_at_a_chunk_edge(post_max):
    case = C.post_max_case(post_max)
    out = run(case)
    check_placed(case, out)
    assert out['meta'][0].tolist() == [post_max, min(post_max, 10)]
    assert np.array_equal(out['idx'][0], case['rank_anchor'][0][:post_max])
    assert (out['idx'][1, 10:] == -1).all() and not out['boxes'][1, 10:].any() and not out['scores'][1, 10:].any()


def test_nonfinite_candidate_in_a_later_lane():
    case = C.nonfinite_case()
    out = run(case)
    check_placed(case, out)
    assert out['meta'][2].tolist() == [NONFINITE, 0]
    mine = case['rank_anchor'][0]
    got = out['idx'][0, :out['meta'][0, 0]].tolist()
    assert mine[200] not in got and mine[201] in got and mine[202] not in got
    assert np.isinf(out['cand_boxes'][0, 200, 3])


def test_iou_exactly_at_the_threshold():
    """IoU == iou_thr does not suppress (the mask bit is IoU > iou_thr)."""
    case = C.exact_threshold_case()
    out = run(case)
    check_placed(case, out)
    assert out['meta'][0].tolist() == [8, 7]


# ---- full size, workspace, repeatability ------------------------------------------------------------------------------------
GUARD = 4096


def _workspace(fill):
    """The cached 'detect' workspace grown to the full-size case's bytes + GUARD and filled with ``fill``; (buffer, bytes)."""
    from modules import Extension as X
    from modules import _hip
    full = C.full_case()
    nbytes = X.lib.mvx_detect_workspace_bytes(full['F'], full['N'], full['pre_max'])
    ws = _hip.workspace(nbytes + GUARD, DEV, 'detect')
    ws.fill_(fill)
    return ws, nbytes


@functools.lru_cache(maxsize=None)
def _full_run():
    """The full-size case once, on a workspace filled with 0xA5: (outputs, the GUARD bytes past the workspace afterwards)."""
    case = C.full_case()
    ws, nbytes = _workspace(0xA5)
    out = run(case, 'rows')
    from modules import _hip
    assert _hip.workspace(nbytes, DEV, 'detect').data_ptr() == ws.data_ptr()        # the call used this buffer
    return out, ws[nbytes:nbytes + GUARD].cpu().numpy()


def test_full_size_matches_the_near_reference():
    """g4224, pre_max = post_max = 4096, two frames (NW = 64, P = 4096, 64 scan chunks of 64 mask words).  The reference,
    detect_ref.greedy_nms_near, takes 0.6 s for a 4096-box frame of this field on the CPU, measured (the full 4096 x 4096 table:
    21 s); about 1230 of the 4096 are kept."""
    case = C.full_case()
    out, _ = _full_run()
    refs = check_selection(case, out)
    assert out['meta'][1].tolist() == [4224, 4096] and [len(r) for r in refs] == [4096, 4096]
    check_nms(case, out, refs, near=True)
    assert (out['meta'][0] >= 300).all()


def test_nothing_is_written_past_the_workspace():
    _, tail = _full_run()
    assert tail.shape == (GUARD,) and (tail == 0xA5).all()


def test_full_size_runs_are_bitwise_equal():
    first, _ = _full_run()
    again = run(C.full_case(), 'rows')
    for k in first:
        a, b = first[k], again[k]
        if k in ('cand_boxes', 'cand_corners'):
            assert (first['cand_idx'] >= 0).all()
        assert same(a, b), k


def test_stale_workspace_bits_are_never_read():
    """n_sel = 65 inside a workspace sized for the full case: a 0xFF-filled buffer and a zeroed one give the same bits."""
    case = C.word_edge_case(65)
    outs = []
    for fill in (0xFF, 0x00):
        _workspace(fill)
        outs.append(run(case, 'rows'))
    check_placed(case, outs[0])
    for k in outs[0]:
        a, b = outs[0][k], outs[1][k]
        if k in ('cand_boxes', 'cand_corners'):
            a, b = a[:, :65], b[:, :65]
        assert same(a, b), k
