"""The learner's conv_precision switch on the host side (no GPU): the parsing of HipLearner's argument, the header's field and constants against
the ctypes mirror, and the references tests/test_gpu_split_learner.py holds the split-bf16 learner conv to -- the integer classes stay exact in
float32 on that file's shapes, and the data-gradient reference (the forward conv with the transposed, tap-flipped weights) is autograd's input
gradient."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conv_layer_cases as cc
from helpers import REPO

HEADER = os.path.join(REPO, 'include', 'mzlearner.h')

# (board, cin_real, cin, num_actions, cout, batch): the single-conv shapes of tests/test_gpu_split_learner.py and what each is there for
INT_SHAPES = {
    'b3_9to16_n5': (3, 9, 9, 0, 16, 5),         # G > 1, hw not a multiple of 4, batch not a multiple of G
    'b5_40to24_n7': (5, 40, 40, 0, 24, 7),      # channel counts off 32 and 16
    'b6_128to128_n3': (6, 128, 128, 0, 128, 3),  # two output-channel blocks, four 32-channel blocks
    'b9_8to8_n1': (9, 8, 8, 0, 8, 1),
    'b13_24to24_n2': (13, 24, 24, 0, 24, 2),
    'b15_35to20_n2': (15, 35, 35, 0, 20, 2),    # the SIDE build
    'b9_32a82to32_n3': (9, 32, 114, 82, 32, 3),  # forward only: 82 action planes generated while staging
}


def flip_transpose(w):
    """The data gradient's weights: [cin, cout, 3, 3], taps flipped -- g = conv(dy, flip_transpose(w))."""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def int_case(cls, shape, direction):
    """(x, action, xf, draws): the integer input of class `cls` for a shape and a direction, the full input the reference convolves, and the
    weight draws AS THE HOOK TAKES THEM ([cout, cin, 3, 3] of the forward layer, either direction)."""
    board, cr, cin, A, cout, B = INT_SHAPES[shape]
    seed = 11 * sorted(INT_SHAPES).index(shape) + 3 * sorted(cc.INT_CLASSES).index(cls) + direction
    if direction == 0:
        x = cc.int_input(cls, 400 + seed, B, cr, board, board)
        action = (np.arange(B) * 37 % A).astype(np.int32) if A else None
        return x, action, cc.full_input(x, action, A, cin), cc.int_draws(cls, 500 + seed, cin, cout)
    # data gradient: the "layer" is cout -> cin with weights flip_transpose(w); the draws are made for THAT layer (three of ITS input channels per
    # draw, every (channel, tap) covered) and handed to the hook in the forward layer's layout
    dy = cc.int_input(cls, 400 + seed, B, cout, board, board)
    draws = [(flip_transpose(wd), b) for wd, b in cc.int_draws(cls, 500 + seed, cout, cin)]  # flip_transpose is its own inverse
    return dy, None, dy, draws


def test_conv_precision_parsing():
    from muzero_amd import hip_learner as hl

    assert hl.CONV_PRECISIONS == {'f32': 0, 'bf16x3': 1}
    for v, want in (('f32', 0), ('bf16x3', 1), (0, 0), (1, 1), (np.int64(1), 1)):
        assert hl._conv_precision(v) == want
    for bad in ('bf16', 'fp32', 2, -1, None, 1.5, True):
        with pytest.raises(ValueError, match='conv_precision'):
            hl._conv_precision(bad)
        with pytest.raises(ValueError, match='conv_precision'):  # refused before anything touches the GPU or the network
            hl.HipLearner(None, 'cuda', 5, 4, lr=1e-3, conv_precision=bad)


def _header_config_fields():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mzl_config\s*;', text).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            assert typ == 'int32_t'
            fields += [n.strip() for n in names.split(',')]
    return fields


def test_header_and_ctypes_mirror_carry_the_field_last():
    from muzero_amd import hip_learner as hl

    text = open(HEADER).read()
    assert re.search(r'^#define\s+MZL_CONV_F32\s+0\b', text, flags=re.M)
    assert re.search(r'^#define\s+MZL_CONV_BF16X3\s+1\b', text, flags=re.M)
    fields = _header_config_fields()
    assert fields[-1] == 'conv_precision' and fields[-2] == 'num_res_blocks'
    assert [n for n, _ in hl.MzlConfig._fields_] == fields
    assert all(t is C.c_int32 for _, t in hl.MzlConfig._fields_)
    assert C.sizeof(hl.MzlConfig) == 4 * len(fields) and hl.MzlConfig.conv_precision.offset == 4 * (len(fields) - 1)
    assert hl.MzlConfig().conv_precision == 0  # a zero-initialised config stays float32
    # the diagnostic hooks are exported, not declared
    for hook in ('mzl_debug_conv', 'mzl_debug_wgrad', 'mzl_debug_conv_fused'):
        assert hook not in re.sub(r'/\*.*?\*/', '', text, flags=re.S) and hook not in hl.ABI_SYMBOLS


RUNS = [(c, s, d) for c in cc.INT_CLASSES for s in INT_SHAPES for d in (0, 1) if not (d == 1 and INT_SHAPES[s][3])]


@pytest.mark.parametrize('cls,shape,direction', RUNS)
def test_integer_classes_stay_exact_on_the_learner_shapes(cls, shape, direction):
    """Zero bias: sum |x||w| < 2^23 and the same over the bf16 terms < 2^24 -- every partial sum of every order, term by term, is an exact
    float32.  True by construction (27 nonzero weights of at most 18 bits, or 8 products of 10 x 10 bits, per output); kept true here."""
    _, _, xf, draws = int_case(cls, shape, direction)
    ref_w = (lambda w: flip_transpose(w)) if direction else (lambda w: w)
    assert cc.covered([(ref_w(w), b) for w, b in draws]).all()
    for i, (w, _) in enumerate(draws):
        plain, terms = cc.int_bounds(xf, ref_w(w), np.zeros(w.shape[1 if direction else 0], np.float32))
        assert plain < 2 ** 23 and terms < 2 ** 24, (cls, shape, direction, i, plain, terms)


def test_data_gradient_reference_is_autograds_input_gradient():
    import torch
    import torch.nn.functional as F

    rs = np.random.RandomState(3)
    B, cin, cout, h, w = 2, 5, 7, 4, 6
    x = torch.from_numpy(rs.randn(B, cin, h, w)).requires_grad_(True)
    wt = rs.randn(cout, cin, 3, 3)
    dy = rs.randn(B, cout, h, w)
    y = F.conv2d(x, torch.from_numpy(wt), padding=1)
    (g,) = torch.autograd.grad(y, x, torch.from_numpy(dy))
    ref = cc.conv_acc(dy, flip_transpose(wt), np.float64)
    assert ref.shape == (B, cin, h, w)
    np.testing.assert_allclose(ref, g.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(flip_transpose(flip_transpose(wt)), wt)
