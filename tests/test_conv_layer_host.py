"""The bars of tests/test_gpu_conv_layer.py discriminate -- shown on the CPU, with tests/conv_layer_cases.py's emulation of the split-bf16
conv (muzero_amd/csrc/mz_conv_split.h): six bf16 term products hh, hm, mh, hl, lh, mm per float32 product, accumulated exactly.

1. On the random data of the accuracy test the six terms are at most a tenth of a float32 chain's error against float64, and the path with
   ANY one term missing is above the GPU test's bar of twice the chain.
2. The three integer classes of the exact test are exact under the six terms in every summation order, the three dropped terms are
   identically zero on them, and every term a class is meant to exercise changes an output when it is dropped."""
import numpy as np
import pytest
import torch

import conv_layer_cases as cc

GPU_BAR = 2.0  # tests/test_gpu_conv_layer.py: E(kernel) <= GPU_BAR * E(chain32)
INT_SHAPE = dict(B=2, cin=40, cout=48, h=9, w=9)  # the generic-build shape of the GPU test


# ------------------------------------------------------------------------------------------ 0. the references themselves
def test_conv64_and_chain32_are_the_layer():
    """conv64 against torch's float64 conv2d on the concatenated input (action planes from muzero_amd.network's own closed form), with
    bias, residual and ReLU; chain32 within float32 rounding of it, and equal to it on integer data."""
    from muzero_amd.network import reference_action_planes

    B, cr, A, cout, h, w = 3, 5, 11, 7, 4, 6
    d = cc.random_layer(3, B, cr, cr + A, cout, h, w, num_actions=A)
    planes = reference_action_planes(torch.from_numpy(d['action']), A, h, w, torch.float64)
    np.testing.assert_array_equal(planes.numpy(), cc.action_planes(d['action'], A, A, h, w))
    xin = torch.cat([torch.from_numpy(d['x']).double(), planes], dim=1)
    for relu in (False, True):
        ref = torch.nn.functional.conv2d(xin, torch.from_numpy(d['w']).double(), torch.from_numpy(d['bias']).double(), padding=1) + \
            torch.from_numpy(d['residual']).double()
        ref = torch.relu(ref) if relu else ref
        kw = dict(bias=d['bias'], action=d['action'], num_actions=A, cin=cr + A, residual=d['residual'], relu=relu)
        np.testing.assert_allclose(cc.conv64(d['x'], d['w'], **kw), ref.numpy(), rtol=1e-13, atol=1e-14)
        c32 = cc.chain32(d['x'], d['w'], **kw)
        assert c32.dtype == np.float32
        np.testing.assert_allclose(c32, ref.numpy(), rtol=0, atol=2e-6)
    xi = cc.int_input('M', 1, 2, 6, 5, 5)
    wi, bi = cc.int_draws('M', 2, 6, 4)[3]
    np.testing.assert_array_equal(cc.chain32(xi, wi, bias=bi), cc.int_reference(xi, wi, bi).astype(np.float32))


def test_split3_is_exact_and_bf16():
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.randn(4096) * 10.0 ** rs.randint(-6, 6, 4096), [0.0, 1.0, -1.0, 262143.0, 1023.0]]).astype(np.float32)
    for t in cc.split3(x):  # (split3 asserts h + m + l == x)
        assert np.array_equal(t.astype(np.float32).view(np.uint32) & 0xffff, np.zeros(len(x), np.uint32)), 'a term is no bf16 value'


# ------------------------------------------------------------------------------------------ 1. random data: the 2 x chain32 bar
@pytest.mark.parametrize('K', [81, 288, 1152])
def test_six_terms_are_float32_grade_and_five_are_not(K):
    x, w = cc.random_dots(K, K)
    ref = (x.astype(np.float64) * w.astype(np.float64)).sum(1)
    scale = np.sqrt((ref ** 2).mean())
    err = lambda v: float(np.sqrt(((v - ref) ** 2).mean()) / scale)  # noqa: E731
    e32 = err(cc.chain32_dots(x, w))
    X, W = cc.split3(x), cc.split3(w)
    six = err(cc.dots_emul(X, W, list(cc.TERMS)))
    five = {n: err(cc.dots_emul(X, W, [t for t in cc.TERMS if t != n])) for n in cc.TERMS}
    print(f'K={K}: chain32 {e32:.3g}, six terms {six:.3g} ({six / e32:.3f} x), without one term: ' +
          ', '.join(f'{n} {v:.3g} ({v / e32:.2f} x)' for n, v in five.items()))
    assert six <= 0.1 * e32
    for n, v in five.items():
        assert v > GPU_BAR * e32, f'K={K}: the path without {n} ({v:.3g}) passes the bar of {GPU_BAR} x chain32 ({e32:.3g})'


# ------------------------------------------------------------------------------------------ 2. integer data: exact
@pytest.fixture(scope='module', params=list(cc.INT_CLASSES))
def int_class(request):
    s = INT_SHAPE
    cls = request.param
    return cls, cc.int_input(cls, 100, s['B'], s['cin'], s['h'], s['w']), cc.int_draws(cls, 101, s['cin'], s['cout'])


def test_integer_classes_are_exact_in_any_order(int_class):
    cls, x, draws = int_class
    c = cc.INT_CLASSES[cls]
    assert c['xmax'] / 2 < np.abs(x).max() <= c['xmax'] and (x != 0).mean() > 0.6
    assert cc.covered(draws).all(), 'a (input channel, tap) of an output channel never carries a weight'
    worst = [0, 0]
    for w, bias in draws:
        nz = (w != 0).reshape(w.shape[0], -1).sum(1)
        assert nz.max() <= c['nnz'] and np.abs(w).max() <= c['wmax'] and len(cc._live(w)) <= 3
        plain, terms = cc.int_bounds(x, w, bias)
        worst = [max(worst[0], plain), max(worst[1], terms)]
        assert plain < 2 ** 23 and terms < 2 ** 24
        ref = cc.int_reference(x, w, bias)
        np.testing.assert_array_equal(cc.split_emul(x, w, exact=True) + bias.astype(np.int64).reshape(1, -1, 1, 1), ref)
        assert not cc.split_emul(x, w, tuple(cc.DROPPED), exact=True).any(), 'a dropped term (ml, lm, ll) is not zero'
        assert np.array_equal(ref.astype(np.float32).astype(np.int64), ref)
    print(f'class {cls}: {len(draws)} draws, max sum |x||w| + |bias| = {worst[0]:.4g} (2^23 = {2 ** 23:.4g}), term by term {worst[1]:.4g} (2^24 = {2 ** 24:.4g})')


def test_every_term_a_class_needs_changes_an_output(int_class):
    cls, x, draws = int_class
    needs = cc.INT_CLASSES[cls]['needs']
    for w, _ in draws[:8]:
        full = cc.split_emul(x, w, exact=True)
        for n in cc.TERMS:
            without = cc.split_emul(x, w, tuple(t for t in cc.TERMS if t != n), exact=True)
            changed = (without != full).mean()
            if n in needs:  # ... in every output channel: the term is exercised across the whole w3 stream of the draw's channels
                assert (without != full).any(axis=(0, 2, 3)).all(), f'class {cls}: dropping {n} leaves an output channel unchanged'
                assert changed > 0.5, f'class {cls}: dropping {n} changes only {changed:.0%} of the outputs'
            else:
                assert changed == 0, f'class {cls} is not meant to need {n}'
