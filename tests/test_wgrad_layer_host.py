"""The references and data of tests/test_gpu_wgrad_layer.py, checked without a GPU (tests/wgrad_layer_cases.py): wgrad64 is float64 autograd's
weight gradient of conv2d(padding=1) -- plain, with action planes, with the two staging transforms, with the ring mask; the integer classes
stay exact in float32 in any summation order on every shape the GPU file runs; the Locator visits the positions its case needs; and every
mistake the weight-gradient kernel could plausibly make (MUTATIONS) changes the integer reference on every shape where it can occur."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_layer_cases as cc
import wgrad_layer_cases as wc
from helpers import REPO
from test_gpu_conv_layer import BAR, MIN_SLICE


# ------------------------------------------------------------------------------------------ the hook's place in the ABI
def test_hook_is_exported_not_declared_and_its_argument_block_is_mirrored():
    from muzero_amd import hip_learner as hl

    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mzlearner.h')).read(), flags=re.S)
    assert 'mzl_debug_wgrad' not in text and 'mzl_debug_wgrad' not in hl.ABI_SYMBOLS
    host = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_learn_conv_host.h')).read()
    for struct, mirror in (('mzl_wgrad_layer', hl.MzlWgradLayer), ('mzl_wgrad_call', hl.MzlWgradCall)):
        body = re.search(r'struct\s+%s\s*\{(.*?)\n\};' % struct, host, flags=re.S).group(1)
        body = re.sub(r'//[^\n]*', '', body)
        names = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                names += [re.sub(r'\[\d+\]', '', n).strip(' *') for n in decl.split(None, 2 if decl.startswith('const') else 1)[-1].split(',')]
        assert names == [n for n, _ in mirror._fields_], (struct, names)
    assert C.sizeof(hl.MzlWgradLayer) == 8 * 8 + 4 * 4 and C.sizeof(hl.MzlWgradCall) == 14 * 4 + 2 * C.sizeof(hl.MzlWgradLayer)
    src = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'learner.hip')).read()
    assert re.search(r'extern "C" int mzl_debug_wgrad\(', src)


# ------------------------------------------------------------------------------------------ the reference is autograd's
def _autograd(dy, xf):
    w = torch.zeros(dy.shape[1], xf.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(torch.from_numpy(np.ascontiguousarray(xf, np.float64)), w, padding=1)
    (g,) = torch.autograd.grad(out, w, torch.from_numpy(np.ascontiguousarray(dy, np.float64)))
    return g.numpy()


def test_wgrad64_is_autograds_weight_gradient():
    rs = np.random.RandomState(7)
    B, cr, cout, h, w, A = 3, 5, 7, 4, 6, 25
    dz, x, y = rs.randn(B, cout, h, w), rs.randn(B, cr, h, w), rs.randn(B, cout, h, w)
    np.testing.assert_allclose(wc.wgrad64(dz, x), _autograd(dz, x), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(wc.model(dz, x, sg=2, ipw=2), _autograd(dz, x), rtol=1e-12, atol=1e-12)
    # action planes (network.py:440-444 written with torch ops)
    action = np.array([3, 24, 0])
    cin = cr + 9
    planes = (torch.arange(9 * h * w).reshape(1, 9, h, w) % A == torch.from_numpy(action).reshape(-1, 1, 1, 1)).double()
    xf = torch.cat([torch.from_numpy(x), planes], dim=1).numpy()
    np.testing.assert_allclose(wc.wgrad64(dz, x, action=action, num_actions=A, cin=cin), _autograd(dz, xf), rtol=1e-12, atol=1e-12)
    # the two transforms as torch ops
    dcoef, xcoef = rs.randn(3, cout), rs.randn(2, cr)
    t = torch.from_numpy
    dy = t(dcoef[0]).reshape(1, -1, 1, 1) * t(dz) + t(dcoef[1]).reshape(1, -1, 1, 1) * t(y) + t(dcoef[2]).reshape(1, -1, 1, 1)
    xt = torch.relu(t(xcoef[0]).reshape(1, -1, 1, 1) * t(x) + t(xcoef[1]).reshape(1, -1, 1, 1))
    np.testing.assert_allclose(wc.wgrad64(dz, x, y=y, dcoef=dcoef, xcoef=xcoef), _autograd(dy.numpy(), xt.numpy()), rtol=1e-12, atol=1e-12)
    assert float((xt == 0).double().mean()) > 0.2  # (the ReLU really cut)
    # the ring mask
    m = torch.zeros(h, w, dtype=torch.float64)
    m[1:-1, 1:-1] = 1
    np.testing.assert_allclose(wc.wgrad64(dz, x, ring=True), _autograd((t(dz) * m).numpy(), x), rtol=1e-12, atol=1e-12)
    # the int64 twin and the float32 chain on integers
    dzi, xi = wc.dense_draw(1, B, cr, cout, h, w)
    ref = wc.wgrad64(dzi, xi, dtype=np.int64)
    assert ref.dtype == np.int64 and np.array_equal(ref, _autograd(dzi, xi)) and np.array_equal(wc.chain32(dzi, xi), ref)
    # a tap mask moves the accumulator taps to the parity plane's weight taps and leaves the rest at the preload
    pre = rs.randn(cout, cr, 3, 3)
    for mask in wc.TAPMASKS:
        out = wc.apply_tapmask(wc.wgrad64(dz, x), mask, pre)
        n = bin(mask).count('1')
        assert int((out != pre).reshape(-1, 9).any(axis=0).sum()) == n and int((out == pre).reshape(-1, 9).all(axis=0).sum()) == 9 - n


# ------------------------------------------------------------------------------------------ every run of the GPU file, as plain data
# (class, draw index, dz, x, kw of the reference) for the integer launches of tests/test_gpu_wgrad_layer.py
def shape_cases(key, sg=1, ipw=1):
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    kw = dict(action=wc.actions(B, A), num_actions=A, cin=cin) if A else {}
    return [(cls, i, dz, x, kw) for cls in wc.CLASSES for i, (dz, x) in enumerate(wc.int_draws(key, cls, sg, ipw))]


def plain_cases(rid):
    run = wc.PLAIN_RUNS[rid]
    return shape_cases(run['shape'], run['expect']['sg'], run['expect']['ipw'])


def transform_cases(rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    d = wc.wide_transform_draw(wc._seed(run['shape'], 'wide', 7), B, cr, cout, board, board)
    return [('wide', 0, d['dz'], d['x'], dict(y=d['y'], dcoef=d['dcoef'])), ('wide', 1, d['dz'], d['x'], dict(y=d['y'], dcoef=d['dcoef'], xcoef=d['xcoef']))]


def tile_cases(key):
    return [(cls, i, dz, x, dict(ring=True)) for cls in wc.CLASSES for i, (dz, x) in enumerate(wc.tile_draws(key, cls))]


INT_IDS = [rid for rid in wc.PLAIN_RUNS if not wc.PLAIN_RUNS[rid]['over'] or rid in wc.ACCUMULATE_RUNS or rid in wc.TRANSFORM_RUNS] + \
          [r + '-transform' for r in wc.TRANSFORM_RUNS] + list(wc.ATARI_TILES) + ['pairs-and-steps']


@pytest.mark.parametrize('rid', INT_IDS)
def test_integer_classes_are_exact_in_float32_in_any_order(rid):
    """sum |dy x'| < 2^24 for every output element, the transformed operands integers below 2^24: whatever the order of the kernel's chunks, rounds,
    MFMA steps and reduce, every partial sum is an exact float32.  (The forced-SG / forced-ipw runs reuse the dense and wide data of their shape;
    their Locators differ in the one-hot positions only: bound = one x value.)  `pairs-and-steps`: the steps' sources are drawn as nsrc x B images
    of the same classes: the bound over all of them."""
    if rid == 'pairs-and-steps':
        cases = []
        for key, nsrc, over, _ in wc.STEP_RUNS.values():
            board, cr, cin, A, cout, B = wc.SHAPES[key]
            cases += [(c, i, dz.reshape((-1,) + dz.shape[2:]), x.reshape((-1,) + x.shape[2:]), {}) for c, i, dz, x in steps_data(key, nsrc)]
        for first, second, _, expect in wc.PAIR_RUNS.values():
            cases += shape_cases(first, *expect[:2]) + shape_cases(second, *expect[:2])
    elif rid.endswith('-transform'):
        cases = transform_cases(rid[:-len('-transform')])
    elif rid in wc.ATARI_TILES:
        cases = tile_cases(rid)
    else:
        cases = plain_cases(rid)
    assert cases
    for cls, i, dz, x, kw in cases:
        bound, dmax, xmax, whole = wc.int_bound(dz, x, **kw)
        assert whole and bound < 2 ** 24 and dmax < 2 ** 24 and xmax < 2 ** 24, (rid, cls, i, bound, dmax, xmax)
        if cls == 'wide' and not kw.get('ring'):
            assert bound > 2 ** 21, (rid, cls, i, bound)  # (it does need most of the mantissa)


def steps_data(key, nsrc):
    """[(class, draw, dz [nsrc, B, ..], x [nsrc, B, ..])]: the classes' draws of an nsrc * B batch, cut into sources."""
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    out = []
    loc = wc.locator_draws(key, nsrc * B, cr, cout, board, board, 1, 1)
    data = [('locator', loc), ('dense', [wc.dense_draw(wc._seed(key, 'dense', nsrc), nsrc * B, cr, cout, board, board)]),
            ('wide', wc.wide_draws(wc._seed(key, 'wide', nsrc), nsrc * B, cr, cout, board, board))]
    for cls, draws in data:
        for i, (dz, x) in enumerate(draws):
            out.append((cls, i, dz.reshape(nsrc, B, cout, board, board), x.reshape(nsrc, B, cr, board, board)))
    return out


# ------------------------------------------------------------------------------------------ the Locator goes where its case needs it
@pytest.mark.parametrize('rid', list(wc.PLAIN_RUNS))
def test_locator_covers_corners_edges_slots_short_rounds_and_short_chunks(rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    sg, ipw = run['expect']['sg'], run['expect']['ipw']
    h = w = board
    draws = wc.int_draws(run['shape'], 'locator', sg, ipw)
    assert 1 <= len(draws) <= 6
    seen = wc.locator_visited(draws)
    pos = {p for _, p in seen}
    for dz, _ in draws:  # one-hot per output channel
        assert np.array_equal(dz.reshape(B, cout, -1).sum(axis=(0, 2)), np.ones(cout)) and set(np.unique(dz)) <= {0.0, 1.0}
    for r, c in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert r * w + c in pos, ('corner', r, c)
    assert any(p // w == 0 and 0 < p % w < w - 1 for p in pos) and any(p // w == h - 1 and 0 < p % w < w - 1 for p in pos)
    assert any(p % w == 0 and 0 < p // w < h - 1 for p in pos) and any(p % w == w - 1 and 0 < p // w < h - 1 for p in pos)
    assert h * w - 1 in pos  # (the last pixel: the quad that straddles the image end when hw % 4 != 0)
    st = wc.structure(B, sg, ipw)
    slot = {b: rnd.index(b) for ch in st for rnd in ch for b in rnd}
    slots_used = max(len(rnd) for ch in st for rnd in ch)
    for gi in range(slots_used):  # first and last column of every image slot of a round: a leak over the separator is seen from both sides
        assert any(slot[b] == gi and p % w == 0 for b, p in seen), ('first column of slot', gi)
        assert any(slot[b] == gi and p % w == w - 1 for b, p in seen), ('last column of slot', gi)
        assert any(slot[b] == gi and p // w == 0 for b, p in seen), ('first row of slot', gi)  # (stacked: the separator is a zero row)
        assert any(slot[b] == gi and p // w == h - 1 for b, p in seen), ('last row of slot', gi)
    short = [rnd for ch in st for rnd in ch if len(rnd) < sg]
    if short:
        assert any(b in rnd for rnd in short for b, _ in seen), 'no image of a short round'
    if B % ipw:
        last = [b for rnd in st[-1] for b in rnd]
        assert any(b == last[0] for b, _ in seen) and any(b == last[-1] for b, _ in seen), 'first and last image of the short last chunk'
    # the value names its source
    x = draws[0][1]
    assert len(np.unique(x)) == x.size and x.min() >= 1
    assert wc.locate(x[B - 1, cr - 1, h - 1, 0], B, cr, h, w) == f'x[image {B - 1}][channel {cr - 1}][({h - 1}, 0)]'


def test_the_named_edges_exist_in_the_case_table():
    """The 6 x 6 runs the issue names: a short last chunk AND a short last round (ipw 8: 8 + 3, the 3 a short round), a chunk of one image (ipw 5),
    ipw 1, SG and B; the update's own SG = 5 choice; both action routes on both action shapes."""
    B = wc.SHAPES['b6_128to128_n11'][5]
    st = wc.structure(B, 4, 8)
    assert [sum(map(len, ch)) for ch in st] == [8, 3] and len(st[-1][-1]) == 3
    assert [sum(map(len, ch)) for ch in wc.structure(B, 4, 5)] == [5, 5, 1] and [len(r) for r in wc.structure(B, 4, 5)[0]] == [4, 1]
    assert {wc.PLAIN_RUNS[f'b6_128to128_n11-sg4-ipw{i}']['over']['ipw'] for i in (1, 4, 11, 5, 8)} == {1, 4, B, 5, 8}
    assert wc.PLAIN_RUNS['b6_128to128_n73']['expect']['sg'] == 5 and wc.PLAIN_RUNS['b6_128to128_n128']['expect']['sg'] == 4
    for rid, sg in (('b6_128to128_n73', 5), ('b3_9to16_n2003', 8)):  # the update's own choice: a short last chunk whose round is short, no override
        st = wc.structure(wc.SHAPES[rid][5], sg, sg)
        assert not wc.PLAIN_RUNS[rid]['over'] and len(st[-1]) == 1 and len(st[-1][0]) == 3 and all(len(ch[0]) == sg for ch in st[:-1])
    acts = {(r['shape'], r['expect']['act']) for r in wc.PLAIN_RUNS.values() if r['expect']['act'] != 'none'}
    assert acts == {(s, a) for s in ('b9_32a82to32_n5', 'b3_16a10to16_n5') for a in ('sparse', 'kernel')}
    for s in wc.SG_LIMITS:
        assert wc.SHAPES[s][5] % 2 == 1 and all(f'{s}-sg{k}-{lay}' in wc.PLAIN_RUNS for lay, n in zip(('cols', 'rows'), wc.SG_LIMITS[s]) for k in range(1, n + 1))


# ------------------------------------------------------------------------------------------ every mistake shows
def _applies(mut, run, shape):
    board, cr, cin, A, cout, B = shape
    sg, ipw = run['expect']['sg'], run['expect']['ipw']
    st = wc.structure(B, sg, ipw)
    if mut == 'stale_idle_slot':
        return any(ri > 0 and len(rnd) < len(ch[ri - 1]) for ch in st for ri, rnd in enumerate(ch))
    if mut == 'separator_leak':
        return run['expect']['layout'] == 'cols' and any(len(rnd) > 1 for ch in st for rnd in ch)
    if mut == 'action_plus_one':
        return A > 0
    if mut == 'transpose_tile':
        return True
    if mut in ('ring_not_zeroed', 'ring_rows_shift', 'ignore_accumulate'):
        return False  # (their own tests below)
    return True


# (3 x 3 above SG = 5: the whole batch is one short round, as at 5; batch 128 and the remap switch: the shape and chunking of batch 73 / 8)
MUT_RUNS = [r for r in wc.PLAIN_RUNS if not re.search(r'-sg([6-9]|1\d)-', r) and 'n128' not in r and not r.endswith('remap-off')]


@pytest.mark.parametrize('rid', MUT_RUNS)
def test_every_mutation_changes_the_integer_reference(rid):
    run = wc.PLAIN_RUNS[rid]
    shape = wc.SHAPES[run['shape']]
    sg, ipw, cols = run['expect']['sg'], run['expect']['ipw'], run['expect']['layout'] != 'rows'
    cases = plain_cases(rid)
    refs = [wc.wgrad64(dz, x, **kw) for _, _, dz, x, kw in cases]
    cases = [(cls, i, dz, x, dict(kw, img=wc.wgrad_images(*wc.transform(dz, x, **kw)))) for cls, i, dz, x, kw in cases]  # (every image's share: once per case)
    for (cls, i, dz, x, kw), ref in zip(cases, refs):
        assert np.array_equal(wc.model(dz, x, sg=sg, ipw=ipw, cols=cols, **kw), ref)  # the unbroken model is the reference
    detected = []
    for mut in wc.MUTATIONS:
        if not _applies(mut, run, shape):
            continue
        hit = [f'{cls}[{i}]' for (cls, i, dz, x, kw), ref in zip(cases, refs) if not np.array_equal(wc.model(dz, x, sg=sg, ipw=ipw, cols=cols, mutation=mut, **kw), ref)]
        assert hit, f'{rid}: mutation {mut} changes no integer reference'
        detected.append(f'{mut}: {",".join(hit)}')
    print(f'{rid}: ' + '; '.join(detected))
    assert {'drop_last_image_of_chunk', 'swap_dx', 'transpose_tile', 'drop_chunk', 'double_chunk'} <= {d.split(':')[0] for d in detected}


def test_stale_slot_and_separator_mutations_have_shapes_where_they_apply():
    for mut in ('stale_idle_slot', 'separator_leak', 'action_plus_one'):
        assert sum(_applies(mut, wc.PLAIN_RUNS[r], wc.SHAPES[wc.PLAIN_RUNS[r]['shape']]) for r in MUT_RUNS) >= 3, mut


@pytest.mark.parametrize('rid', wc.ACCUMULATE_RUNS)
def test_ignoring_accumulate_changes_the_reference(rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    pre = preload(cout, cin)
    assert np.all(pre != 0)
    for cls, i, dz, x, kw in plain_cases(rid):
        ref = wc.wgrad64(dz, x, **kw) + pre
        assert np.array_equal(wc.model(dz, x, preload=pre, accumulate=True, **kw), ref)
        assert np.all(wc.model(dz, x, preload=pre, accumulate=True, mutation='ignore_accumulate', **kw) != ref)
        assert wc.int_bound(dz, x, **kw)[0] + np.abs(pre).max() < 2 ** 24


def preload(cout, cin):
    """A non-zero integer for every element of the output."""
    v = (np.arange(cout * cin * 9) % 199 + 1) * np.where(np.arange(cout * cin * 9) % 3 == 0, -1, 1)
    return v.reshape(cout, cin, 3, 3).astype(np.float32)


@pytest.mark.parametrize('key', list(wc.ATARI_TILES))
def test_ring_mutations_change_the_reference(key):
    cases = [(cls, i, dz, x, dict(kw, img=wc.wgrad_images(*wc.transform(dz, x, **kw)))) for cls, i, dz, x, kw in tile_cases(key)]
    refs = {(cls, i): kw['img'].sum(axis=0) for cls, i, dz, x, kw in cases}
    for mut in ('ring_not_zeroed', 'ring_rows_shift', 'swap_dx', 'transpose_tile', 'drop_last_image_of_chunk'):
        hit = [f'{cls}[{i}]' for cls, i, dz, x, kw in cases if not np.array_equal(wc.model(dz, x, mutation=mut, **kw), refs[cls, i])]
        assert hit, (key, mut)
        if mut in ('ring_not_zeroed', 'ring_rows_shift'):
            assert any(h.startswith('locator') for h in hit), (key, mut, hit)  # the Locator names the pixel
    # the Locator's ring pixels contribute nothing, and the tile's rows 0 and h - 1 of x are read through the dy = -1 / +1 taps
    h, w, cr, cout, B = wc.ATARI_TILES[key]
    zero_rows = top = bottom = 0
    for dz, x in wc.tile_draws(key, 'locator'):
        ref = wc.wgrad64(dz, x, ring=True)
        for b, co, r, c in np.argwhere(dz != 0):
            on_ring = r in (0, h - 1) or c in (0, w - 1)
            assert (not ref[co].any()) == on_ring
            zero_rows += on_ring
            if not on_ring and r == 1:
                assert ref[co, 0, 0, 1] == x[b, 0, 0, c]
                top += 1
            if not on_ring and r == h - 2:
                assert ref[co, 0, 2, 1] == x[b, 0, h - 1, c]
                bottom += 1
    assert zero_rows >= 8 and top >= 3 and bottom >= 3


# ------------------------------------------------------------------------------------------ the random bar rejects a lost image and a stale slot
def test_random_bar_rejects_a_dropped_image_and_a_stale_slot():
    rs = np.random.RandomState(11)
    B, cin, cout, board = 11, 32, 32, 6
    x, dz = cc.random_values(rs, (B, cin, board, board), (B, cout, board, board))
    ref = wc.wgrad64(dz, x)
    c32 = wc.chain32(dz, x)
    assert min(cin * 9, cout * 9, cin * cout) >= MIN_SLICE
    for mut in ('drop_last_image_of_chunk', 'stale_idle_slot'):
        bad = wc.model(dz, x, sg=4, ipw=5, mutation=mut)
        for s, ax in wc.SLICES.items():
            e, ec = cc.rel_rms(bad, ref, ax), cc.rel_rms(c32, ref, ax)
            assert np.all(ec > 0) and np.all(e > BAR * ec), (mut, s)
    for s, ax in wc.SLICES.items():  # and the unbroken model in float32-free float64 passes it trivially
        assert np.all(cc.rel_rms(wc.model(dz, x, sg=4, ipw=5), ref, ax) <= BAR * cc.rel_rms(c32, ref, ax))
