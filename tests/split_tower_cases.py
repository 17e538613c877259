"""A residual tower (conv-ReLU-conv, + block input, ReLU; n_convs = 2 * blocks) on the CPU, layer by layer on tests/conv_layer_cases.py: the
float64 reference, the float32 chain yardstick, an emulation of the split-bf16 tower (muzero_amd/csrc/mz_tower_split.h) and the data of
tests/test_split_tower_host.py and tests/test_gpu_split_tower.py.  numpy only: importable without a GPU.

x [B, P, h, w], weights [n_convs, P, P, 3, 3], biases [n_convs, P]."""
import functools

import numpy as np

from conv_layer_cases import TERMS, bf16, chain32, conv_acc, int_pool, split3, split_emul

F32 = np.float32


def _bias(b, dtype):
    return np.asarray(b).astype(dtype).reshape(1, -1, 1, 1)


def tower64(x, weights, biases):
    """float64 throughout (the float32 inputs' values, no rounding anywhere between the layers)."""
    x = np.asarray(x, np.float64)
    for i in range(0, len(weights), 2):
        t = np.maximum(conv_acc(x, weights[i], np.float64) + _bias(biases[i], np.float64), 0.0)
        x = np.maximum(conv_acc(t, weights[i + 1], np.float64) + _bias(biases[i + 1], np.float64) + x, 0.0)
    return x


def tower_chain32(x, weights, biases):
    """The yardstick: every layer ONE float32 chain per output (conv_layer_cases.chain32), float32 residual add, ReLU."""
    x = np.asarray(x, F32)
    for i in range(0, len(weights), 2):
        t = chain32(x, weights[i], biases[i], relu=True)
        x = chain32(t, weights[i + 1], biases[i + 1], residual=x, relu=True)
        assert x.dtype == F32
    return x


def tower_emul(x, weights, biases, terms=tuple(TERMS), residual='f32', exact=False, pre=None):
    """The split tower: every layer the sum of the chosen bf16 term products (float64, or int64 with exact=True) + bias, rounded to float32;
    + residual in float32; ReLU; the result split again by the next layer.  residual: 'f32' the block input (the kernel), 'bf16' its high
    bf16 term, 'wrong_block' the input of the block before (block 0: its own).  pre: a list that receives every pre-activation."""
    x = np.asarray(x, F32)
    prev_in = x
    for i in range(0, len(weights), 2):
        a = (split_emul(x, weights[i], terms, exact) + _bias(biases[i], np.int64 if exact else np.float64))
        res = {'f32': x, 'bf16': bf16(x), 'wrong_block': prev_in}[residual]
        t = np.maximum(a, 0).astype(F32)
        b = split_emul(t, weights[i + 1], terms, exact) + _bias(biases[i + 1], np.int64 if exact else np.float64)
        b = b + res.astype(b.dtype) if exact else (b.astype(F32) + res).astype(np.float64)
        if pre is not None:
            pre += [a, b]
        prev_in = x
        x = np.maximum(b, 0).astype(F32)
    return x


def tower_int(x, weights, biases, pre=None):
    """int64 throughout."""
    x = np.asarray(x).astype(np.int64)
    for i in range(0, len(weights), 2):
        a = conv_acc(x, weights[i], np.int64) + _bias(biases[i], np.int64)
        b = conv_acc(np.maximum(a, 0), weights[i + 1], np.int64) + _bias(biases[i + 1], np.int64) + x
        if pre is not None:
            pre += [a, b]
        x = np.maximum(b, 0)
    return x


# ------------------------------------------------------------------------------------------ random data
@functools.lru_cache(maxsize=None)
def random_tower(seed, B, P, h, w, n_convs):
    """x ~ U[0, 1) with 40 % exact zeros, w ~ N(0, 2 / (9 P)) (the activations keep their scale through the tower), bias ~ N(0, 0.1^2)."""
    rs = np.random.RandomState(seed)
    x = (rs.uniform(0, 1, (B, P, h, w)) * (rs.rand(B, P, h, w) < 0.6)).astype(F32)
    weights = (rs.randn(n_convs, P, P, 3, 3) * np.sqrt(2.0 / (9 * P))).astype(F32)
    biases = (rs.randn(n_convs, P) * 0.1).astype(F32)
    for a in (x, weights, biases):
        a.setflags(write=False)
    return x, weights, biases


@functools.lru_cache(maxsize=None)
def random_references(seed, B, P, h, w, n_convs):
    """(float64 tower, float32 chain tower) of random_tower's data, computed once and shared."""
    x, weights, biases = random_tower(seed, B, P, h, w, n_convs)
    r64, r32 = tower64(x, weights, biases), tower_chain32(x, weights, biases)
    r64.setflags(write=False)
    r32.setflags(write=False)
    return r64, r32


# ------------------------------------------------------------------------------------------ integer data, two blocks
# Inputs 0 / 1; two nonzero weights per output channel.  Channels fall in three classes (channel % 3) that only read their own class, so the
# magnitudes stay apart:  class 0 -- 18-bit weights (h, m, l) on the 0 / 1 input in conv 0, then +-1 on the resulting 19..22-bit
# activations (h, m, l): the terms hh hm hl, then hh mh lh;  class 1 -- 10-bit weights (h, m) in conv 0 AND conv 1, whose inputs are then
# 11-bit activations (h, m): the term mm;  class 2 -- weights +-1..3 on small activations.  No pair of operands has a nonzero product among
# the three cross terms the kernel drops (ml, lm, ll), so the six issued terms sum to the int64 result.
INT_CONVS = 4


@functools.lru_cache(maxsize=None)
def int_tower(seed, B, P, h, w):
    """(x, weights, biases) float32 with integer values, INT_CONVS convs."""
    rs = np.random.RandomState(seed)
    x = (rs.rand(B, P, h, w) < 0.5).astype(F32)
    weights = np.zeros((INT_CONVS, P, P, 9), F32)
    biases = rs.randint(-3, 4, (INT_CONVS, P)).astype(F32)
    small = np.array([1, 2, 3], F32)
    for cv in range(INT_CONVS):
        for co in range(P):
            cls = co % 3
            pool = (int_pool((1 << 18) - 1) if cv == 0 else np.ones(1, F32)) if cls == 0 else \
                (int_pool((1 << 10) - 1) if cv < 2 else np.ones(1, F32)) if cls == 1 else small
            nnz = 1 if (cls == 1 and cv >= 2) else 2
            chans = np.arange(cls, P, 3)
            for _ in range(nnz):
                weights[cv, co, rs.choice(chans), rs.randint(9)] = rs.choice(pool) * (1 if rs.rand() < 0.45 else -1)
    weights = weights.reshape(INT_CONVS, P, P, 3, 3)
    for a in (x, weights, biases):
        a.setflags(write=False)
    return x, weights, biases


def int_tower_bound(x, weights, biases):
    """max over layers and outputs of |bias| + sum of every |x term| * |w term| (+ |residual|): below 2^24, every partial sum of every
    summation order, term by term, is an exact float32."""
    x = np.asarray(x).astype(np.int64)
    worst = 0
    for i in range(0, len(weights), 2):
        for j, (inp, res) in enumerate(((x, None), (None, x))):
            if inp is None:
                inp = t
            X, W = split3(inp.astype(F32)), split3(weights[i + j])
            m = conv_acc(sum(np.abs(v) for v in X), sum(np.abs(v) for v in W), np.int64) + np.abs(_bias(biases[i + j], np.int64))
            if res is not None:
                m = m + np.abs(res)
            worst = max(worst, int(m.max()))
            a = conv_acc(inp, weights[i + j], np.int64) + _bias(biases[i + j], np.int64) + (0 if res is None else res)
            if j == 0:
                t = np.maximum(a, 0)
            else:
                x = np.maximum(a, 0)
    return worst
