"""The split-bf16 weight gradient without a GPU (tests/wgrad_split_cases.py): the numpy model of k_lc_wgrad_bf16x3 EQUALS the int64 reference on the
integer classes of every shape tests/test_gpu_wgrad_split.py launches, every one of its six terms is needed on the Wide class, the random bar
accepts the six-term model and rejects a two-term one, the Locator visits the positions whose dx = -1 / +1 neighbour crosses a lane group, a
dword or a step, the geometry written down here agrees with the float32 tables wherever the two kernels must agree, and the switch parses."""
import os
import re

import numpy as np
import pytest

import conv_layer_cases as cc
import wgrad_layer_cases as wc
import wgrad_split_cases as sc
from test_gpu_conv_layer import BAR, MIN_SLICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, sg, ipw, rows) of every integer launch of the GPU file, once each
MODEL_RUNS = sorted({(wc.PLAIN_RUNS[r]['shape'], sc.expect_plain(r)['sg'], sc.expect_plain(r)['ipw'], False) for r in sc.PLAIN_IDS} |
                    {(k, sg, sc.images_per_chunk(wc.SHAPES[k][5], sg, wc.SHAPES[k][4], wc.SHAPES[k][1]), lay == 2) for k, lay, sg in sc.SG_RUNS})


def _model_kw(key, sg, ipw, rows):
    return dict(sg=sg, ipw=ipw, rows=rows)


@pytest.mark.parametrize('key,sg,ipw,rows', MODEL_RUNS, ids=[f'{k}-sg{s}-ipw{i}-{"rows" if r else "cols"}' for k, s, i, r in MODEL_RUNS])
def test_model_equals_int64_on_the_integer_classes(key, sg, ipw, rows):
    for cls, i, dz, x, kw, ref in sc.int_cases(key, sg, ipw, rows):
        bound, dmax, xmax, whole = wc.int_bound(dz, x, **kw)
        assert whole and bound < 2 ** 24 and dmax < 2 ** 24 and xmax < 2 ** 24, (key, cls, i, bound)
        if cls in ('locator', 'locator8') and (key.startswith('b6_128') or key.startswith('b13') or key.startswith('b15')) and i > 0:
            continue  # (the model is slow on the large shapes: one Locator draw of each kind there; the GPU runs all)
        out = sc.model(dz, x, exact=True, **_model_kw(key, sg, ipw, rows), **kw)
        assert wc.first_difference(out, ref) is None, (key, cls, i, wc.first_difference(out, ref))


WIDE_SHAPES = sorted({wc.PLAIN_RUNS[r]['shape'] for r in sc.PLAIN_IDS})


@pytest.mark.parametrize('key', WIDE_SHAPES)
def test_every_dropped_term_changes_the_wide_reference(key):
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    kw = dict(action=wc.actions(B, A), num_actions=A, cin=cin) if A else {}
    draws = wc.int_draws(key, 'wide')
    refs = [wc.wgrad64(dz, x, dtype=np.int64, **kw) for dz, x in draws]
    for drop in sc.TERMS:
        terms = tuple(t for t in sc.TERMS if t != drop)
        assert any(not np.array_equal(sc.model(dz, x, sg=1, ipw=B, terms=terms, exact=True, **kw), ref) for (dz, x), ref in zip(draws, refs)), (key, drop)


def test_float32_model_matches_the_exact_one_on_integers():
    key = 'b5_40to24_n7'
    for cls, i, dz, x, kw, ref in sc.int_cases(key, 3, 7):
        assert np.array_equal(sc.model(dz, x, sg=3, ipw=7, **kw), ref.astype(np.float32)), (cls, i)


RANDOM_HOST = {'b9_40to48': (9, 40, 48, 25), 'b15_64to80': (15, 64, 80, 10)}  # tests/test_gpu_wgrad_layer.py RANDOM_CASES, same seeds


@pytest.mark.parametrize('cid', list(RANDOM_HOST))
def test_bar_accepts_six_terms_and_rejects_two(cid):
    board, cin, cout, B = RANDOM_HOST[cid]
    rs = np.random.RandomState(3000 + board * board + cin)
    x, dz = cc.random_values(rs, (B, cin, board, board), (B, cout, board, board))
    ref, c32 = wc.wgrad64(dz, x), wc.chain32(dz, x)
    assert min(cin * 9, cout * 9, cin * cout) >= MIN_SLICE
    g = sc.geom(board, board, B, cout, cin)
    ipw = sc.images_per_chunk(B, g['sg'], cout, cin)
    six = sc.model(dz, x, sg=g['sg'], ipw=ipw)
    two = sc.model(dz, x, sg=g['sg'], ipw=ipw, terms=('hh', 'hm', 'mh', 'mm'))  # the operands cut to h + m: 16 bits each
    for s, ax in wc.SLICES.items():
        e6, e2, ec = cc.rel_rms(six, ref, ax), cc.rel_rms(two, ref, ax), cc.rel_rms(c32, ref, ax)
        assert np.all(e6 <= BAR * ec), (cid, s, float(np.max(e6 / ec)))
        assert np.all(e2 > BAR * ec), (cid, s, float(np.min(e2 / ec)))


@pytest.mark.parametrize('key,sg,ipw,rows', MODEL_RUNS, ids=[f'{k}-sg{s}-ipw{i}-{"rows" if r else "cols"}' for k, s, i, r in MODEL_RUNS])
def test_locator_visits_group_dword_and_step_crossings_in_every_slot(key, sg, ipw, rows):
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    P = sc.planes(board, board, sg, rows)[0]
    draws = sc.locator_draws(key, sg, ipw, rows)
    seen = wc.locator_visited(draws)
    assert set(sc.locator_required(board, board, B, sg, ipw, rows)) <= seen
    big = max((rnd for ch in wc.structure(B, sg, ipw) for rnd in ch), key=len)
    assert len(big) == min(sg, B, ipw)
    for gi, b in enumerate(big):
        fs = {((gi * (board + 1) + p // board) * P + p % board if (rows and sg > 1) else (p // board) * P + gi * (board + 1) + p % board) for bb, p in seen if bb == b}
        every = {((gi * (board + 1) + p // board) * P + p % board if (rows and sg > 1) else (p // board) * P + gi * (board + 1) + p % board) for p in range(board * board)}
        if board * board <= 36:
            assert fs == every, (key, gi)
        # a neighbour in another lane's group or another step (f % 8 in {0, 7}), in another dword inside a group ({1, 2}): every such position of the slot
        assert {f for f in every if f % 8 in (0, 1, 2, 7)} <= fs, (key, gi)
        assert any(f % 2 == 0 for f in fs) and any(f % 2 == 1 for f in fs)
        assert {f for f in every if f % 32 in (0, 31)} <= fs, (key, gi)  # (a neighbour in another step: among the f % 8 in {0, 7})


def test_geometry_follows_the_code():
    # 15 x 15: pitch 16, 8 steps of 32 (256 slots for 225 pixels), 111 232 bytes: one workgroup per CU, a second image per round does not fit
    assert sc.planes(15, 15, 1, False) == (16, 8, 264, 312, 640 + 192 * 576)
    assert sc.geom(15, 15, 128, 128, 128)['sg'] == 1 and sc.geom(15, 15, 3, 20, 35, sg=2) is None
    # 6 x 6: side by side 7 images (56 columns, 11 steps) are 163 456 of the 163 840 bytes, and the staging lanes hold no eighth (9 quads each)
    assert sc.planes(6, 6, 7, False)[:2] == (56, 11) and sc.planes(6, 6, 7, False)[4] == 163456 <= sc.LDS_MAX
    assert sc.sg_limit('b6_128to128_n11', 1) == 7 and sc.sg_limit('b3_9to16_n5', 1) == 16
    # 5 x 5 (7 quads): 9 images fill the lanes; stacked, 8 x 6 - 1 rows of pitch 8 fit and 9 x 6 - 1 do not
    assert sc.sg_limit('b5_40to24_n7', 1) == 9 and sc.sg_limit('b5_40to24_n7', 2) == 8
    for key, lay, sg in sc.SG_REFUSED:
        board, cr, cin, A, cout, B = wc.SHAPES[key]
        assert sc.geom(board, board, B, cout, cr, sg, lay) is None and (sg == 1 or sc.geom(board, board, B, cout, cr, sg - 1, lay) is not None)
    # every stride keeps 16-byte reads aligned and the planes inside the LDS
    for h in range(1, 16):
        for sg in range(1, 17):
            for rows in (False, True):
                P, ns, spy, spx, lds = sc.planes(h, h, sg, rows)
                assert P % 8 == 0 and spy % 8 == 0 and spx % 8 == 0 and spy % 16 == 8 and spx % 16 == 8
                assert 32 * ns >= (sg * (h + 1) - 1 if rows and sg > 1 else h) * P
                # the furthest element a lane reads: step ns - 1, kq 3, row +1, the right neighbour dword
                assert 32 * (ns - 1) + 24 + 2 * P + 8 + 8 + 1 < spx and 32 * ns <= spy
                # the spare slots that elements past the image and idle lanes are stored to: dy index 32 ns, x index spx - 2, neither ever read
                assert 32 * ns < spy and 32 * (ns - 1) + 24 + 2 * P + 8 + 8 + 1 < spx - 2


def test_forced_runs_agree_with_the_float32_tables():
    """Where SG and ipw are forced, or the split path picks the float32 kernel's SG, chunking is Sched::wgrad_ops' either way: the expectations
    written down here must equal tests/wgrad_layer_cases.py's."""
    for rid in sc.PLAIN_IDS:
        e, f = sc.expect_plain(rid), wc.PLAIN_RUNS[rid]['expect']
        if 'sg' in wc.PLAIN_RUNS[rid]['over'] or e['sg'] == f['sg']:
            assert (e['sg'], e['layout'], e['ipw'], e['act']) == (f['sg'], f['layout'], f['ipw'], f['act']), rid
    for pid, (_, _, over, want) in wc.PAIR_RUNS.items():
        if 'sg' in over or sc.expect_pair(pid)[0] == want[0]:
            assert sc.expect_pair(pid) == want, pid
    for sid, (_, _, over, want) in wc.STEP_RUNS.items():
        if 'sg' in over or sc.expect_steps(sid)[0] == want[0]:
            assert sc.expect_steps(sid) == want, sid
    # where the split planes pick another SG than the float32 ones (one workgroup per CU; two 6 x 6 images fill a 16-wide pitch no worse than one fills 8)
    assert sc.expect_pair('different_grids')[:2] == (2, 2) and sc.expect_plain('b3_9to16_n5')['sg'] == 2


def test_wgrad_precision_parses_like_conv_precision():
    from muzero_amd import hip_learner as hlm

    assert hlm.WGRAD_PRECISIONS == {'f32': 0, 'bf16x3': 1}
    assert [hlm._wgrad_precision(v) for v in ('f32', 'bf16x3', 0, 1)] == [0, 1, 0, 1]
    for bad in (2, -1, 'bf16', 'F32', None, True, 1.5, '1'):
        with pytest.raises(ValueError, match='wgrad_precision'):
            hlm._wgrad_precision(bad)


def test_header_declares_the_constants_and_the_setter():
    from muzero_amd import hip_learner as hlm

    with open(os.path.join(ROOT, 'include', 'mzlearner.h')) as f:
        text = f.read()
    assert re.search(r'#define\s+MZL_WGRAD_F32\s+0\b', text) and re.search(r'#define\s+MZL_WGRAD_BF16X3\s+1\b', text)
    assert re.search(r'int\s+mzl_set_wgrad_precision\(mz_learner\*\s*h,\s*int32_t\s+precision\);', text)
    assert 'mzl_set_wgrad_precision' in hlm.ABI_SYMBOLS
    assert text.index('mzl_set_wgrad_precision(') < text.index('int mzl_bind(')  # (declared where it is legal: between create and bind)


def test_hip_learner_refuses_a_bad_value_before_touching_the_gpu():
    from muzero_amd.hip_learner import HipLearner

    with pytest.raises(ValueError, match='wgrad_precision'):
        HipLearner(None, 'cuda:0', 5, 4, lr=1e-3, wgrad_precision='bf16')
