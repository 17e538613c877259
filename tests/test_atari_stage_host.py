"""CPU-side checks of tests/atari_stage_cases.py, the references and data of tests/test_gpu_atari_stage.py: the route models of the stride-2 conv and its
data gradient equal the direct int64 sums on the committed data; the references agree with PyTorch's float64 convs, pools and the autograd of
normalize_hidden_state; every planted mistake (MUTATIONS) changes a checked value on a NAMED committed case, so the GPU test's equality on that case
would catch the same mistake in a kernel; the preconditions that make equality the right assertion hold (2^24 bounds, d exact); and the hook's symbol
is handled like mzl_debug_conv_tile's."""
import os
import re

import numpy as np
import pytest

import atari_stage_cases as ac
from helpers import REPO

LIMIT = 1 << 24


# ------------------------------------------------------------------------------------------ stride-2 conv and data gradient
@pytest.mark.parametrize('shape', ac.S2_FWD, ids=str)
def test_s2_route_model_equals_the_direct_sum(shape):
    for cls in ac.S2_CLASSES:
        x, ws = ac.s2_case(cls, shape)
        for w in ws:
            assert ac.s2_bound(x, w) < LIMIT
            ref = ac.s2_direct(x, w)
            for wide in (True, False):
                assert np.array_equal(ac.s2_route(x, w, wide=wide), ref), (cls, wide)
        if cls == 'locator':  # every output channel reads one tap, the draws' channels cover all nine
            taps = {int(np.flatnonzero(w[co].reshape(w.shape[1], 9).sum(0))[0]) for w in ws for co in range(w.shape[0])}
            assert taps == set(range(9))


@pytest.mark.parametrize('shape', ac.S2_DGRAD + (ac.S2_DGRAD_WIDE,), ids=str)
def test_s2_dgrad_route_model_equals_the_direct_sum(shape):
    for cls in ac.S2_CLASSES:
        dy, ws = ac.s2_case(cls, shape, dgrad=True)
        for w in ws:
            assert ac.s2_bound(dy, w, dgrad=True) < LIMIT
            ref = ac.s2_dgrad_direct(dy, w)
            for wide in (True, False):
                assert np.array_equal(ac.s2_dgrad_route(dy, w, wide=wide), ref), (cls, wide)


def test_tap_masks_are_the_dispatchers():
    assert ac.FWD_MASKS == (0x010, 0x018, 0x012, 0x01b)
    assert ac.DGRAD_MASKS == (0x010, 0x030, 0x090, 0x1b0)
    src = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'learner_conv.hip')).read()
    for m in set(ac.FWD_MASKS + ac.DGRAD_MASKS):
        assert 'MZ_CT(15, 0x%03x)' % m in src  # (the table of builds, kConvBuilds: one entry per tap set at NPT 15)


def test_s2_references_agree_with_torch_float64():
    import torch
    import torch.nn.functional as F

    x, (w,) = ac.s2_case('small', ac.S2_FWD[2])
    xt, wt = torch.tensor(x, dtype=torch.float64, requires_grad=True), torch.tensor(w, dtype=torch.float64)
    y = F.conv2d(xt, wt, stride=2, padding=1)
    assert np.array_equal(y.detach().numpy(), ac.s2_direct(x, w).astype(np.float64))
    dy, (w2,) = ac.s2_case('small', ac.S2_DGRAD[0], dgrad=True)
    cin, cout, H, W, B = ac.S2_DGRAD[0]
    xin = torch.zeros(B, cin, 2 * H, 2 * W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, torch.tensor(w2, dtype=torch.float64), stride=2, padding=1).backward(torch.tensor(dy, dtype=torch.float64))
    assert np.array_equal(xin.grad.numpy(), ac.s2_dgrad_direct(dy, w2).astype(np.float64))


# ------------------------------------------------------------------------------------------ pools, ReLU backward
@pytest.mark.parametrize('hw', ac.POOLS, ids=str)
def test_pool_references_agree_with_torch_float64(hw):
    import torch
    import torch.nn.functional as F

    x, g = ac.pool_case(hw)
    assert x.size % 256 and g.size % 256
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = F.avg_pool2d(xt, 3, 2, 1)
    y.backward(torch.tensor(g, dtype=torch.float64))
    fwd, bwd = ac.pool_fwd_ref(x), ac.pool_bwd_ref(g)
    assert fwd.dtype == bwd.dtype == np.float32 and fwd.shape == y.shape and bwd.shape == x.shape
    assert np.abs(fwd - y.detach().numpy()).max() <= 2.0 ** -24 * np.abs(y.detach().numpy()).max()  # (one float32 rounding of the quotient)
    assert np.abs(bwd - xt.grad.numpy()).max() <= 2.0 ** -24 * np.abs(xt.grad.numpy()).max()


def test_relu_case_holds_the_signed_zeros_and_a_subnormal():
    g, x = ac.relu_case()
    assert g.size == 1000
    bits = x.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any() and (bits == 1).any() and (bits == 0x80000001).any()
    ref = ac.relu_bwd_ref(g, x)
    assert np.array_equal(ref[bits == 1], g[bits == 1]) and not ref[bits == 0].any() and not ref[bits == 0x80000000].any()


# ------------------------------------------------------------------------------------------ entry, normalize
def test_entry_reference_agrees_with_the_autograd_of_normalize_hidden_state():
    """Tie-free data only: torch's amin / amax share a tied gradient among the attaining channels, the kernel (and torch's min(dim) / max(dim)) give it
    to the first."""
    import torch

    from muzero_amd.network import normalize_hidden_state

    rs = np.random.RandomState(5)
    for C in (8, 13, 24):
        x = (rs.rand(2, C, 36) + 0.5).astype(np.float32)
        gs = rs.randn(2, C, 36).astype(np.float32)
        assert all(len(np.unique(x[b, :, p])) == C for b in range(2) for p in range(36))
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        s = normalize_hidden_state(xt)
        s.backward(torch.tensor(gs, dtype=torch.float64) * 0.5)
        ref = ac.entry_ref(x, gs, 0.5, None, np.zeros_like(x), d_rule='f64')
        assert np.allclose(ref['dz'], xt.grad.numpy(), rtol=1e-11, atol=1e-11)
        assert np.abs(ac.normalize_ref(x) - s.detach().numpy()).max() < 1e-6


@pytest.mark.parametrize('C', ac.ENTRY_C)
def test_exact_entry_classes_meet_their_preconditions(C):
    cpt, ng = ac.channel_groups(C)
    for cls in ac.EXACT_CLASSES:
        for B, n in ((1, 36), (3, 144), (3, 2304)):
            case = ac.entry_case(cls, B, C, n)
            x = case['x']
            mn, mx = x.min(1), x.max(1)
            assert np.array_equal(x, np.rint(x)) and set(np.unique(mx - mn)) <= {1.0, 2.0, 4.0, 8.0}
            assert (mn >= 1).mean() >= 0.5 and (mn == 0).any()
            zero_px = mn == 0
            assert ((x == 0).sum(1)[zero_px] >= 2).mean() > 0.5 if cls == 'pow2' else True  # several zero channels where the minimum is 0
            for scale in (0.5, 1.0):
                d_exact, dyadic, bound = ac.entry_exactness(case, scale, True)
                assert d_exact and dyadic and bound < LIMIT, (cls, B, n, scale, bound)
            if cls == 'ties':
                at_min, at_max = x == mn[:, None], x == mx[:, None]
                assert (at_min.sum(1) >= 2).mean() > 0.6 and (at_max.sum(1) >= 2).mean() > 0.6
                group = np.arange(C) // cpt
                first_min = at_min.argmax(1)
                gmin = [np.unique(group[at_min[b, :, p]]) for b in range(B) for p in range(min(n, 144))]
                if cpt >= 2:
                    assert any(len(g) == 1 and g[0] < ng - 1 for g in gmin)          # inside one thread's channel run
                assert any(len(g) >= 2 for g in gmin)                                # in different channel groups
                assert (group[first_min] == ng - 1).any()                            # the lowest attaining channel in the last group
                assert (group[at_max.argmax(1)] == ng - 1).any()


# ------------------------------------------------------------------------------------------ every mutation is caught by a named case
def _s2_differs(shape, cls, bug, wide=True):
    x, ws = ac.s2_case(cls, shape)
    return any(not np.array_equal(ac.s2_route(x, w, wide=wide, bug=bug), ac.s2_direct(x, w)) for w in ws)


def _dgrad_differs(shape, cls, bug):
    dy, ws = ac.s2_case(cls, shape, dgrad=True)
    return any(not np.array_equal(ac.s2_dgrad_route(dy, w, bug=bug), ac.s2_dgrad_direct(dy, w)) for w in ws)


def _entry_differs(cls, B, C, n, scale, extra, bug):
    case = ac.entry_case(cls, B, C, n)
    e = case['extra'] if extra else None
    a, b = ac.entry_ref(case['x'], case['gs'], scale, e, case['partner']), ac.entry_ref(case['x'], case['gs'], scale, e, case['partner'], bug=bug)
    return not np.array_equal(a['dz'].astype(np.float32), b['dz'].astype(np.float32))


def _gather_differs(mode, inner_only, bug):
    src0, src1, coef = ac.gather_case(2, 5, 24, 24, 1)
    kw = dict(src1=src1, coef=coef, mode=mode, stride=1, origin=(0, 0), inner_only=inner_only, tw=12)
    return not np.array_equal(ac.gather_ref(src0, **kw), ac.gather_ref(src0, bug=bug, **kw))


def _stats_differ(bug):
    tiles, skip = ac.scatter_case(2, 5, 12, 12, 12, False, 1)
    _, v = ac.scatter_ref(tiles, 2, 12, 12, 12, 1, (0, 0), skip, False)
    return not np.array_equal(ac.scatter_stats(v), ac.scatter_stats(v, bug=bug))


# mutation -> (the committed case that catches it, does it?)
CAUGHT_BY = {
    'parity_swapped': ('s2_fwd locator (4, 16, 24, 24, 2)', lambda: _s2_differs(ac.S2_FWD[0], 'locator', 'parity_swapped')),
    'odd_plane_origin': ('s2_fwd locator (4, 16, 24, 24, 2)', lambda: _s2_differs(ac.S2_FWD[0], 'locator', 'odd_plane_origin')),
    'plane_overwrites': ('s2_fwd small (20, 24, 24, 24, 1)', lambda: _s2_differs(ac.S2_FWD[2], 'small', 'plane_overwrites')),
    'edge_repeats': ('s2_fwd locator (3, 16, 48, 48, 1)', lambda: _s2_differs(ac.S2_FWD[1], 'locator', 'edge_repeats')),
    'dgrad_forward_taps': ('s2_dgrad locator (16, 32, 24, 24, 2)', lambda: _dgrad_differs(ac.S2_DGRAD[0], 'locator', 'dgrad_forward_taps')),
    'pool_valid_count': ('pool_fwd (6, 6)', lambda: not np.array_equal(ac.pool_fwd_ref(ac.pool_case((6, 6))[0]), ac.pool_fwd_ref(ac.pool_case((6, 6))[0], bug='pool_valid_count'))),
    'pool_bwd_window': ('pool_bwd (12, 24)', lambda: not np.array_equal(ac.pool_bwd_ref(ac.pool_case((12, 24))[1]), ac.pool_bwd_ref(ac.pool_case((12, 24))[1], bug='pool_bwd_window'))),
    'argmin_last': ('entry ties B=1 C=13 hw=36 scale=1.0', lambda: _entry_differs('ties', 1, 13, 36, 1.0, True, 'argmin_last')),
    'minmax_terms_swapped': ('entry pow2 B=1 C=8 hw=36 scale=1.0', lambda: _entry_differs('pow2', 1, 8, 36, 1.0, False, 'minmax_terms_swapped')),
    'scale_dropped': ('entry pow2 B=1 C=24 hw=144 scale=0.5', lambda: _entry_differs('pow2', 1, 24, 144, 0.5, True, 'scale_dropped')),
    'mask_ge': ('entry pow2 B=3 C=72 hw=36 scale=1.0', lambda: _entry_differs('pow2', 3, 72, 36, 1.0, False, 'mask_ge')),
    'pivot_zero': ('scatter statistics 12 x 12, C = 5, B = 2', lambda: _stats_differ('pivot_zero')),
    'inner_only_ignored': ('gather ident inner_only 24 x 24, C = 5, B = 2', lambda: _gather_differs('ident', True, 'inner_only_ignored')),
    'bnbwd_coef_order': ('gather bnbwd 24 x 24, C = 5, B = 2', lambda: _gather_differs('bnbwd', False, 'bnbwd_coef_order')),
}


@pytest.mark.parametrize('bug', ac.MUTATIONS)
def test_every_mutation_changes_a_checked_value_on_a_named_case(bug):
    case, differs = CAUGHT_BY[bug]
    assert differs(), f'{bug} is not caught by {case}'


def test_mutation_table_is_complete_and_the_models_are_clean_without_a_bug():
    assert sorted(CAUGHT_BY) == sorted(ac.MUTATIONS)
    assert not _s2_differs(ac.S2_FWD[0], 'locator', None) and not _dgrad_differs(ac.S2_DGRAD[0], 'locator', None)
    assert not _entry_differs('ties', 1, 13, 36, 1.0, True, None) and not _stats_differ(None) and not _gather_differs('bnbwd', True, None)


def test_argmin_rule_is_invisible_without_ties_and_mask_rule_without_zeros():
    """Why the classes exist: on tie-free positive data neither the arg-min rule nor the mask rule can be told apart."""
    rs = np.random.RandomState(3)
    x = np.stack([rs.permutation(8) + 1.0 for _ in range(36)], axis=1).reshape(1, 8, 36).astype(np.float32)
    gs = rs.randint(-2, 3, x.shape).astype(np.float32)
    base = ac.entry_ref(x, gs, 1.0, None, gs)['dz']
    for bug in ('argmin_last', 'mask_ge'):
        assert np.array_equal(ac.entry_ref(x, gs, 1.0, None, gs, bug=bug)['dz'], base)


# ------------------------------------------------------------------------------------------ gather, scatter
def test_gather_and_scatter_references_round_trip():
    for tw, W in ((12, 24), (16, 48)):
        src0, src1, coef = ac.gather_case(2, 5, 24, W, 2)
        for origin in ((0, 0), (0, 1), (1, 0), (1, 1)):
            t = ac.gather_ref(src0, None, None, 'ident', 2, origin, False, tw)
            dst, v = ac.scatter_ref(t, 2, 24, W, tw, 2, origin, None, False)
            py, px = origin
            assert np.array_equal(dst[:, :, py::2, px::2], src0[:, :, py::2, px::2]) and np.isnan(dst).sum() == 3 * v.size
    tiles, skip = ac.scatter_case(2, 5, 12, 12, 12, False, 1)
    _, v = ac.scatter_ref(tiles, 2, 12, 12, 12, 1, (0, 0), skip, False)
    st = ac.scatter_stats(v)
    assert st.shape == (2 * 5, 5, 4) and set(st[:, :, 3].ravel()) == {32.0, 16.0}      # 144 positions: the last chunk holds 16
    assert np.abs(st[:, :, 2]).max() < LIMIT
    tot = (st[:, :, 0] * st[:, :, 3] + st[:, :, 1]).reshape(2, 5, 5).sum(1)
    assert np.array_equal(tot, v.sum((2, 3)))


# ------------------------------------------------------------------------------------------ the hook's symbol
def test_hook_is_exported_but_not_declared():
    from muzero_amd import hip_learner as hl

    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mzlearner.h')).read(), flags=re.S)
    for hook in ('mzl_debug_atari_stage', 'mzl_debug_conv_tile'):
        assert hook not in text and hook not in hl.ABI_SYMBOLS
    src = open(os.path.join(REPO, 'muzero_amd', 'hip_learner.py')).read()
    for hook in ('mzl_debug_atari_stage', 'mzl_debug_conv_tile'):  # the same optional binding: a library without the hook still loads
        assert re.search(r"if hasattr\(L, '%s'\):\n\s+L\.%s\.argtypes = \[vp, C\.POINTER\(\w+\), C\.POINTER\(C\.c_char_p\)\]" % (hook, hook), src)
    csrc = os.path.join(REPO, 'muzero_amd', 'csrc')
    assert 'extern "C" int mzl_debug_atari_stage(mz_learner* h, mzl_stage_call* call, const char** build_name)' in open(os.path.join(csrc, 'learner.hip')).read()
    host = open(os.path.join(csrc, 'mz_learn_conv_host.h')).read()
    assert host.index('struct mzl_tile_call') < host.index('struct mzl_stage_call') < host.index('struct mzl_wgrad_layer')


def test_stage_call_layout_matches_the_header():
    import ctypes as C

    from muzero_amd import hip_learner as hl

    host = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_learn_conv_host.h')).read()
    body = host[host.index('struct mzl_stage_call {'):]
    body = re.sub(r'//[^\n]*', '', body[:body.index('};')])
    names = [n.strip() for decl in re.findall(r'(?:int32_t|float\*?|const float\*)\s+([^;]+);', body) for n in decl.split(',')]
    assert names == [n for n, _ in hl.MzlStageCall._fields_]
    assert C.sizeof(hl.MzlStageCall) == 16 * 4 + 8 * 8
    for op, v in hl.STAGE_OPS.items():
        assert re.search(r'MZL_STAGE_%s = %d\b' % (op.upper(), v), host)
    for name, v in hl.ENTRY_LAUNCHERS.items():
        assert re.search(r'MZL_ENTRY_%s = %d\b' % (name.upper(), v), host)
    with pytest.raises(ValueError, match='op must be one of'):
        hl.HipLearner.debug_atari_stage(None, 'conv')
