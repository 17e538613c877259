"""One 3x3 stride-1 conv layer on the CPU: the float64 reference, the float32 yardstick, an emulation of the split-bf16 path
(muzero_amd/csrc/mz_conv_split.h) and the data of tests/test_conv_layer_host.py and tests/test_gpu_conv_layer.py.  numpy only: importable
without a GPU.

Layouts are the planner's: x [B, cin, h, w], w [cout, cin, 3, 3] (cross-correlation, zero padding 1), k = (input channel, tap) with
tap = 3 * ky + kx.  The dynamics net's action planes: element f = c * h * w + pixel of the [planes, h, w] block is 1 iff f % A == action."""
import numpy as np

TERMS = {'hh': (0, 0), 'hm': (0, 1), 'mh': (1, 0), 'hl': (0, 2), 'lh': (2, 0), 'mm': (1, 1)}  # (x term, w term) the kernel issues, in its order
DROPPED = {'ml': (1, 2), 'lm': (2, 1), 'll': (2, 2)}


# ------------------------------------------------------------------------------------------ number formats
def bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m): the three terms as float64 arrays."""
    x = np.asarray(x, dtype=np.float32)
    h = bf16(x)
    r1 = (x - h).astype(np.float32)
    m = bf16(r1)
    r2 = (r1 - m).astype(np.float32)
    l = bf16(r2)  # noqa: E741
    assert np.array_equal(h.astype(np.float64) + m + l, x.astype(np.float64)), 'h + m + l != x'
    return [t.astype(np.float64) for t in (h, m, l)]


# ------------------------------------------------------------------------------------------ the layer
def action_planes(action, num_actions, planes, h, w):
    """[B, planes, h, w] float32 (network.py:440-444)."""
    f = np.arange(planes * h * w).reshape(1, planes, h, w) % num_actions
    return (f == np.asarray(action).reshape(-1, 1, 1, 1)).astype(np.float32)


def full_input(x, action=None, num_actions=0, cin=None):
    """The real channels followed by the generated action planes, up to cin channels."""
    x = np.asarray(x)
    if action is None:
        return x
    B, cr, h, w = x.shape
    return np.concatenate([x, action_planes(action, num_actions, cin - cr, h, w).astype(x.dtype)], axis=1)


def im2col(x):
    """[B, C, h, w] -> [B * h * w, C * 9], column c * 9 + tap."""
    B, C, h, w = x.shape
    xp = np.zeros((B, C, h + 2, w + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    cols = np.stack([xp[:, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], axis=-1)  # [B, C, h, w, 9]
    return np.ascontiguousarray(cols.transpose(0, 2, 3, 1, 4)).reshape(B * h * w, C * 9)


def _to_planes(flat, B, h, w):
    return np.ascontiguousarray(flat.reshape(B, h, w, -1).transpose(0, 3, 1, 2))


def _live(w):
    """Input channels that carry a nonzero weight (the integer draws use three of them)."""
    return np.flatnonzero(np.abs(w).reshape(w.shape[0], w.shape[1], 9).sum(axis=(0, 2)) != 0)


def conv_acc(x, w, dtype):
    """sum_k x * w in `dtype` (float64 or int64), [B, cout, h, w]; only the input channels with a nonzero weight are multiplied."""
    B, _, h, wd = x.shape
    ch = _live(w)
    if len(ch) == 0:
        return np.zeros((B, w.shape[0], h, wd), dtype)
    cols = im2col(np.asarray(x)[:, ch].astype(dtype))
    return _to_planes(cols @ np.asarray(w)[:, ch].astype(dtype).reshape(w.shape[0], -1).T, B, h, wd)


def conv64(x, w, bias=None, action=None, num_actions=0, cin=None, residual=None, relu=False):
    """The layer in float64: im2col + matmul, + bias, + residual, ReLU."""
    out = conv_acc(full_input(np.asarray(x, np.float32), action, num_actions, cin), np.asarray(w, np.float32), np.float64)
    if bias is not None:
        out = out + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    if residual is not None:
        out = out + np.asarray(residual, np.float64)
    return np.maximum(out, 0.0) if relu else out


def chain32(x, w, bias=None, action=None, num_actions=0, cin=None, residual=None, relu=False):
    """The same layer as ONE float32 chain per output, k in (input channel, tap) order from the bias: every product and every add rounded to
    float32 (no fused multiply-add).  The yardstick: what plain float32 arithmetic makes of this data."""
    xf = full_input(np.asarray(x, np.float32), action, num_actions, cin)
    B, C, h, wd = xf.shape
    w = np.asarray(w, np.float32)
    cout = w.shape[0]
    cols, wt = im2col(xf), np.ascontiguousarray(w.reshape(cout, C * 9).T)
    acc = np.zeros((B * h * wd, cout), np.float32)
    if bias is not None:
        acc += np.asarray(bias, np.float32).reshape(1, cout)
    for k in range(C * 9):
        acc = acc + cols[:, k:k + 1] * wt[k:k + 1]
        assert acc.dtype == np.float32
    out = _to_planes(acc, B, h, wd)
    if residual is not None:
        out = out + np.asarray(residual, np.float32)
    return np.maximum(out, np.float32(0)) if relu else out


def split_emul(x, w, terms=tuple(TERMS), exact=False):
    """sum over the chosen (x term, w term) pairs of conv(X_term, W_term), every bf16 product exact: accumulated in float64, or with
    exact=True (integer data) in int64.  No bias."""
    X, W = split3(x), split3(w)
    dtype = np.int64 if exact else np.float64
    if exact:
        assert all(np.array_equal(t, np.rint(t)) for t in X + W), 'exact=True needs integer terms'
    pairs = {**TERMS, **DROPPED}
    out = 0
    for name in terms:
        a, b = pairs[name]
        out = out + conv_acc(X[a], W[b], dtype)
    return out


def dots_emul(X, W, names):
    """The same for plain dot products: X, W = split3 of [N, K] arrays."""
    pairs = {**TERMS, **DROPPED}
    return sum((X[pairs[n][0]] * W[pairs[n][1]]).sum(1) for n in names)


def chain32_dots(x, w):
    acc = np.zeros(x.shape[0], np.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k] * w[:, k]
    assert acc.dtype == np.float32
    return acc


# ------------------------------------------------------------------------------------------ statistics
def rel_rms(out, ref, axes=None):
    """rms(out - ref) / rms(ref) in float64 over `axes` of [B, cout, h, w]: None whole output, (0, 2, 3) per channel, (0, 1) per pixel."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((out - ref) ** 2).mean(axis=axes)) / np.sqrt((ref ** 2).mean(axis=axes))


SLICES = {'whole': None, 'channel': (0, 2, 3), 'pixel': (0, 1)}


# ------------------------------------------------------------------------------------------ random data
def random_values(rs, x_shape, w_shape):
    """x ~ U[0, 1) with 40 % exact zeros (a ReLU'd, normalised hidden state), w ~ N(0, 0.05^2)."""
    x = rs.uniform(0, 1, x_shape).astype(np.float32) * (rs.rand(*x_shape) < 0.6)
    w = (rs.randn(*w_shape) * 0.05).astype(np.float32)
    return x.astype(np.float32), w


def random_dots(seed, K, N=4096):
    """N independent dot products of length K."""
    return random_values(np.random.RandomState(seed), (N, K), (N, K))


def random_layer(seed, B, cin_real, cin, cout, h, w, num_actions=0):
    """dict(x, w, bias, action, residual) of one layer; action is None unless cin > cin_real."""
    rs = np.random.RandomState(seed)
    x, wt = random_values(rs, (B, cin_real, h, w), (cout, cin, 3, 3))
    bias = (rs.randn(cout) * 0.1).astype(np.float32)
    action = rs.randint(0, num_actions, size=B).astype(np.int32) if cin > cin_real else None
    residual = rs.uniform(-1, 1, (B, cout, h, w)).astype(np.float32)
    return dict(x=x, w=wt, bias=bias, action=action, residual=residual)


# ------------------------------------------------------------------------------------------ integer data
# Every value an integer; a draw puts weights on three input channels only.  Class -> (|x| max, |w| max, nonzero weights per output channel
# and draw, the issued terms the class needs).  x = +-1 and w = +-1 have m = l = 0; the 18-bit integers are those that need h, m and l, the
# 10-bit ones those that need h and m (int_pool).
INT_CLASSES = {
    'W': dict(xmax=1, wmax=(1 << 18) - 1, nnz=27, needs=('hh', 'hm', 'hl')),
    'X': dict(xmax=(1 << 18) - 1, wmax=1, nnz=27, needs=('hh', 'mh', 'lh')),
    'M': dict(xmax=(1 << 10) - 1, wmax=(1 << 10) - 1, nnz=8, needs=('hh', 'hm', 'mh', 'mm')),
}
INT_BIAS_MAX = 1000
_POOLS = {}


def int_pool(vmax):
    """The integers in [1, vmax] that need every bf16 term an integer of vmax's size can need: m != 0, and above 16 bits l != 0 as well (an
    18-bit integer that happens to fit h + m would pass through a kernel that lost its l stream)."""
    if vmax not in _POOLS:
        v = np.arange(1, vmax + 1, dtype=np.float32)
        _, m, l = split3(v)  # noqa: E741
        _POOLS[vmax] = v[(m != 0) & (l != 0)] if vmax >= 1 << 16 else (v[m != 0] if vmax > 1 else v)
    return _POOLS[vmax]


def int_input(cls, seed, B, cin_real, h, w):
    """Dense integer activations [B, cin_real, h, w] (float32) of class `cls`."""
    c = INT_CLASSES[cls]
    rs = np.random.RandomState(seed)
    if c['xmax'] == 1:
        return rs.randint(-1, 2, (B, cin_real, h, w)).astype(np.float32)
    x = rs.choice(int_pool(c['xmax']), (B, cin_real, h, w)) * rs.choice([-1, 1], (B, cin_real, h, w))  # dense: every position multiplies
    return x.astype(np.float32)


def int_draws(cls, seed, cin, cout):
    """The weight draws of class `cls` for a cin -> cout layer: a list of (w [cout, cin, 3, 3] float32, bias [cout] float32).  Draw group d
    carries weights on input channels 3d, 3d + 1, 3d + 2 only; where the class allows fewer than 27 nonzero weights per output channel, the
    group is several draws whose nonzero positions partition the 27 (another random partition per output channel).  The union of the draws
    puts a nonzero weight on EVERY (input channel, tap) of EVERY output channel."""
    c = INT_CLASSES[cls]
    rs = np.random.RandomState(seed)
    parts = -(-27 // c['nnz'])
    draws = []
    for d in range(-(-cin // 3)):
        order = np.stack([rs.permutation(27) for _ in range(cout)])  # [cout, 27]: position -> part order[co, pos] % parts
        mag = rs.choice(int_pool(c['wmax']), (cout, 27))
        val = mag * rs.choice([-1, 1], (cout, 27))
        for part in range(parts):
            w3 = np.zeros((cout, cin + 3, 9), np.float32)
            w3[:, 3 * d:3 * d + 3] = np.where(order % parts == part, val, 0).reshape(cout, 3, 9)
            bias = rs.randint(-INT_BIAS_MAX, INT_BIAS_MAX + 1, cout).astype(np.float32)
            draws.append((np.ascontiguousarray(w3[:, :cin]).reshape(cout, cin, 3, 3), bias))
    return draws


def int_bounds(xf, w, bias):
    """(max over outputs of sum |x||w| + |bias|, the same with every |x term| * |w term| product): the first under 2^23 and the second
    under 2^24 make every partial sum of every summation order, term by term, an exact float32."""
    X, W = split3(xf), split3(w)
    plain = conv_acc(np.abs(xf), np.abs(w), np.int64) + np.abs(bias).astype(np.int64).reshape(1, -1, 1, 1)
    terms = conv_acc(sum(np.abs(t) for t in X), sum(np.abs(t) for t in W), np.int64) + np.abs(bias).astype(np.int64).reshape(1, -1, 1, 1)
    return int(plain.max()), int(terms.max())


def int_reference(xf, w, bias):
    """The int64 conv + bias."""
    return conv_acc(xf, w, np.int64) + np.asarray(bias).astype(np.int64).reshape(1, -1, 1, 1)


def covered(draws):
    """[cout, cin, 3, 3] bool: where the union of the draws has a nonzero weight."""
    return np.any([w != 0 for w, _ in draws], axis=0)
