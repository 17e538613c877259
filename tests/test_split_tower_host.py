"""The split-bf16 fused tower (mz_planner_set_tower_precision, muzero_amd/csrc/mz_tower_split.h) without a GPU: the Python surface, the header,
and the data of tests/test_gpu_split_tower.py -- the numpy tower references agree where they must, the integer towers are exact in every
summation order, and the checks the GPU tests apply tell a dropped term or a wrong residual from the kernel's arithmetic."""
import os
import re
import types

import numpy as np
import pytest

import split_tower_cases as stc
from conv_layer_cases import TERMS, rel_rms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'include', 'mzplanner.h')
INT_GEOMETRIES = [(11, 16, 3, 3), (3, 48, 5, 5), (2, 32, 9, 9)]  # (B, P, h, w): the ones tests/test_gpu_split_tower.py runs, smaller batches


# ------------------------------------------------------------------------------------------ the Python surface
def test_tower_precision_parses_names_and_numbers():
    from muzero_amd import planner as pl

    assert pl.TOWER_PRECISIONS == {'f32': 0, 'bf16x3': 1}
    assert [pl._tower_precision(v) for v in ('f32', 'bf16x3', 0, 1, np.int32(1))] == [0, 1, 0, 1, 1]


@pytest.mark.parametrize('bad', ['bf16', 'fp32', '', 2, -1, 0.5, None, True, False, [1]])
def test_unknown_tower_precision_raises(bad):
    from muzero_amd import planner as pl

    with pytest.raises((ValueError, TypeError)) as e:
        pl._tower_precision(bad)
    assert 'tower_precision' in str(e.value) or isinstance(e.value, TypeError)


def test_planner_refuses_a_bad_tower_precision_before_touching_the_library():
    from muzero_amd import planner as pl

    with pytest.raises(ValueError, match='tower_precision'):
        pl.Planner(types.SimpleNamespace(), 0, tower_precision='bf16')


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_constants_and_prototype():
    text = _header()
    assert re.search(r'^#define\s+MZ_TOWER_F32\s+0\b', text, flags=re.M)
    assert re.search(r'^#define\s+MZ_TOWER_BF16X3\s+1\b', text, flags=re.M)
    assert re.search(r'^int\s+mz_planner_set_tower_precision\s*\(\s*mz_planner\s*\*\s*p\s*,\s*int32_t\s+precision\s*\)\s*;', text, flags=re.M)
    assert 'mz_debug_res_tower' not in text  # a test hook: exported, undeclared


def test_abi_symbols_are_the_declared_symbols():
    from muzero_amd import planner as pl

    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = re.findall(r'^\s*(?:const\s+char\s*\*|int|int32_t)\s+(mz_\w+)\s*\(', text, flags=re.M)
    assert sorted(declared) == sorted(pl.ABI_SYMBOLS)
    assert 'mz_planner_set_tower_precision' in pl.ABI_SYMBOLS


# ------------------------------------------------------------------------------------------ the numpy towers
def test_random_tower_references_agree_within_float32():
    x, w, b = stc.random_tower(3, 2, 16, 5, 5, 4)
    r64, r32 = stc.random_references(3, 2, 16, 5, 5, 4)
    assert r64.dtype == np.float64 and r32.dtype == np.float32 and r64.shape == x.shape
    assert 0.2 < np.sqrt((r64 ** 2).mean()) < 20.0 and (r64 > 0).mean() > 0.2  # the tower neither dies nor blows up
    e32 = float(rel_rms(r32, r64))
    assert 0 < e32 < 1e-5
    emul = stc.tower_emul(x, w, b)
    assert float(rel_rms(emul, r64)) < 2.0 * e32  # the six issued terms, summed exactly: at least as close as the float32 chain's bar
    assert float(rel_rms(stc.tower_emul(x, w, b, terms=('hh',)), r64)) > 100 * e32  # bf16 alone is nowhere near


# ------------------------------------------------------------------------------------------ integer towers
@pytest.mark.parametrize('B,P,h,w', INT_GEOMETRIES)
def test_integer_tower_is_exact_in_every_order(B, P, h, w):
    x, wt, bs = stc.int_tower(7, B, P, h, w)
    assert set(np.unique(x)) == {0.0, 1.0} and wt.shape == (stc.INT_CONVS, P, P, 3, 3)
    assert np.array_equal(wt, np.rint(wt)) and (wt != 0).reshape(stc.INT_CONVS, P, -1).sum(-1).max() <= 2  # sparse integers
    assert stc.int_tower_bound(x, wt, bs) < 1 << 24
    pre = []
    ref = stc.tower_int(x, wt, bs, pre=pre)
    assert len(pre) == stc.INT_CONVS
    neg = sum(int((a < 0).sum()) for a in pre) / sum(a.size for a in pre)
    assert neg >= 1 / 3, neg
    assert (ref > 0).mean() > 0.1 and ref.max() > 1 << 16  # alive, and large enough to need all three terms
    emul = stc.tower_emul(x, wt, bs, exact=True)
    np.testing.assert_array_equal(emul.astype(np.int64), ref)


@pytest.mark.parametrize('B,P,h,w', INT_GEOMETRIES)
def test_integer_tower_tells_mistakes_apart(B, P, h, w):
    """The GPU test's check is equality with the int64 tower: each of these mistakes must break it."""
    x, wt, bs = stc.int_tower(7, B, P, h, w)
    ref = stc.tower_int(x, wt, bs)
    for drop in TERMS:
        out = stc.tower_emul(x, wt, bs, terms=tuple(t for t in TERMS if t != drop), exact=True)
        assert not np.array_equal(out.astype(np.int64), ref), f'dropping {drop} goes unnoticed'
    for residual in ('bf16', 'wrong_block'):
        out = stc.tower_emul(x, wt, bs, residual=residual, exact=True)
        assert not np.array_equal(out.astype(np.int64), ref), f'a {residual} residual goes unnoticed'


def test_random_tower_bar_tells_mistakes_apart():
    """The GPU test's bar on random data: 2.0 x the float32 chain's error against float64.  A dropped term or a bf16 residual must miss it."""
    x, w, b = stc.random_tower(3, 2, 16, 5, 5, 4)
    r64, r32 = stc.random_references(3, 2, 16, 5, 5, 4)
    bar = 2.0 * float(rel_rms(r32, r64))
    for drop in TERMS:
        assert float(rel_rms(stc.tower_emul(x, w, b, terms=tuple(t for t in TERMS if t != drop)), r64)) > bar, drop
    for residual in ('bf16', 'wrong_block'):
        assert float(rel_rms(stc.tower_emul(x, w, b, residual=residual), r64)) > bar, residual
