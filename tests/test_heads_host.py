"""The float64 model of the conv learner's head block (tests/heads_cases.py) against float64 autograd through the project's own heads and loss, the
bounds of the data classes tests/test_gpu_heads.py runs, and the reach of that test: every one of a list of deliberate arithmetic mistakes moves the
model somewhere the GPU test looks.  No GPU."""
import numpy as np
import pytest
import torch

import heads_cases as hc
from heads_cases import Geom

f64 = np.float64
# board heads (squared error), Atari heads (categorical) at odd supports, and at EVEN supports (linspace(-half, half, S) has spacing 2 half / (S - 1), not
# 1, there: the model follows the formulas of network.py / learner.py, the autograd side IS those functions)
HOST_GEOMS = {'board': Geom(4, 6, 7, 3, 1, 1), 'atari_odd': Geom(4, 6, 5, 3, 11, 5), 'atari_even': Geom(4, 6, 5, 2, 10, 6), 'mixed': Geom(3, 4, 5, 2, 1, 8)}


class _HeadsOnly:
    """What learner.loss_tensors needs of a network, with the towers replaced by given outputs: the hidden state is the step counter."""

    def __init__(self, g, case):
        from muzero_amd.network import _plane_head
        self.value_support_size, self.reward_support_size = g.Sv, g.Sr
        self.mse_loss_for_value, self.mse_loss_for_reward = g.Sv == 1, g.Sr == 1
        self.mods = []
        for (oc, n, _, _, _), p, (rm, rv), nb in zip(hc.heads(g), case['heads'], case['running'], case['nbt']):
            m = _plane_head(g.P, oc, g.hw, n).double().train()
            sd = {'0.weight': p['w1'].reshape(oc, g.P, 1, 1), '1.weight': p['gamma'], '1.bias': p['beta'], '1.running_mean': rm, '1.running_var': rv,
                  '1.num_batches_tracked': np.int64(nb), '4.weight': p['lw'], '4.bias': p['lb']}
            m.load_state_dict({k: torch.as_tensor(np.asarray(v)).double() if k != '1.num_batches_tracked' else torch.tensor(int(v)) for k, v in sd.items()})
            self.mods.append(m)
        B = len(case['idx'])
        shape = (g.K, B, g.P, 2, g.hw // 2)  # (any h x w with h w = hw: the heads flatten it)
        self.F_pred = torch.tensor(case['F_pred'].reshape(shape), dtype=torch.float64, requires_grad=True)
        self.F_rew = torch.tensor(case['F_rew'].reshape(shape), dtype=torch.float64, requires_grad=True)

    def represent(self, state):
        return torch.zeros(())

    def prediction(self, hidden):
        t = int(hidden.item())
        return self.mods[1](self.F_pred[t]), self.mods[2](self.F_pred[t])

    def dynamics(self, hidden, action):
        t = int(hidden.item())
        return hidden + 1, self.mods[0](self.F_rew[t])


def _autograd(g, case):
    from muzero_amd.learner import loss_tensors
    net = _HeadsOnly(g, case)
    idx = case['idx']
    tt = lambda a: torch.tensor(np.asarray(a, f64))  # noqa: E731
    loss, prio = loss_tensors(net, None, torch.zeros(len(idx), g.K, dtype=torch.long), tt(case['value'][idx]), tt(case['reward'][idx]), tt(case['pi'][idx]), tt(case['w']))
    loss.backward()
    grads = [{k: m.state_dict(keep_vars=True)[key].grad.numpy().reshape(np.shape(case['heads'][i][k]))
              for k, key in (('w1', '0.weight'), ('gamma', '1.weight'), ('beta', '1.bias'), ('lw', '4.weight'), ('lb', '4.bias'))} for i, m in enumerate(net.mods)]
    B = len(idx)
    return dict(loss=float(loss.detach()), prio=prio.numpy(), dF_pred=net.F_pred.grad.numpy().reshape(g.K, B, g.P, g.hw), dF_rew=net.F_rew.grad.numpy().reshape(g.K, B, g.P, g.hw),
                grads=grads, running=[(m[1].running_mean.numpy(), m[1].running_var.numpy()) for m in net.mods], nbt=np.array([int(m[1].num_batches_tracked) for m in net.mods]))


def _close(a, ref, what, tol=1e-12):
    a, ref = np.asarray(a, f64), np.asarray(ref, f64)
    assert a.shape == ref.shape, what
    err = float(np.abs(a - ref).max()) if a.size else 0.0
    assert err <= tol * max(1.0, float(np.abs(ref).max())), f'{what}: off by {err:.3g} (largest |ref| {np.abs(ref).max():.3g})'


@pytest.mark.parametrize('name', sorted(HOST_GEOMS))
@pytest.mark.parametrize('data', ['random', 'edge'])
def test_model_equals_float64_autograd_through_the_projects_heads_and_loss(name, data):
    g = HOST_GEOMS[name]
    case = (hc.random_case if data == 'random' else hc.edge_case)(g, 6, 5)
    m, a = hc.model(case, g), _autograd(g, case)
    _close(m['loss'], a['loss'], 'loss')
    _close(m['prio'], a['prio'], 'priorities')
    _close(m['dF_pred'], a['dF_pred'], 'gradient wrt the prediction tower\'s outputs')
    _close(m['dF_rew'], a['dF_rew'], 'gradient wrt the dynamics tower\'s outputs')
    for hd, hn in enumerate(hc.HEAD_NAMES):
        for k in ('w1', 'gamma', 'beta', 'lw', 'lb'):
            _close(m['grads'][hd][k], a['grads'][hd][k], f'{hn} d{k}')
        _close(m['running'][hd][0], a['running'][hd][0], f'{hn} running_mean after {g.K} steps')
        _close(m['running'][hd][1], a['running'][hd][1], f'{hn} running_var after {g.K} steps')
    assert (m['nbt'] == a['nbt']).all() and (m['nbt'] == case['nbt'] + g.K).all()


def test_support_and_projection_follow_the_reference_formulas_at_odd_and_even_sizes():
    """linspace(-half, half, S) with half = (S - 1) // 2 (util.py:62-67,84-85), and the 2-hot projection's expectation over it gives the clamped
    transformed target back (up to the 1e-5 of its denominator): unit spacing only at odd S."""
    for S in (3, 4, 5, 6, 10, 11, 301):
        sup = hc.support(S, f64)
        half = (S - 1) // 2
        assert sup[0] == -half and sup[-1] == half and np.allclose(np.diff(sup), 2.0 * half / (S - 1), rtol=0, atol=1e-15)
        assert (np.diff(sup) == 1.0).all() == (S % 2 == 1)
        x = np.array([0.0, 0.3, -2.5, 7.0, -40.0, 1e4, -1e4])
        th = hc.two_hot(x, S, f64)
        z = np.clip(hc.signed_hyperbolic(x, f64), -half, half)
        assert ((th > 0).sum(1) <= 2).all() and np.allclose(th.sum(1), 1.0, atol=1e-12)
        if half > 0:
            assert np.allclose(th @ sup, z, atol=2e-5 * max(1, half))


GPU_CASES = [(n, B) for n in sorted(hc.GEOMS) for B in hc.BATCHES[n]]


@pytest.mark.parametrize('name,B', GPU_CASES)
def test_the_gpu_tests_data_meets_its_bounds(name, B):
    """Integer data: every forward sum of absolute terms below 2^24.  Random and edge data, and the parameter variants built on it: every pre-activation
    |a u + b| at least 2^-10 x the case's largest, every element counted."""
    g, seed = hc.GEOMS[name], hc.case_seed(name, B)
    ic = hc.integer_case(g, B, seed)
    assert hc.integer_bound(ic, g) < 2.0 ** 24
    for arr in (ic['F_pred'], ic['F_rew'], ic['heads'][0]['w1'], ic['heads'][1]['w1'], ic['heads'][2]['w1']):
        assert (arr == np.round(arr)).all()
    lo, hi = hc.margin(ic, g)
    assert lo >= hc.MARGIN * hi
    rc = hc.random_case(g, B, seed)
    lo, hi = hc.margin(rc, g)
    assert lo >= hc.MARGIN * hi, f'{name} B={B}: least |a u + b| {lo:.3g} under 2^-10 x {hi:.3g}'
    if B == hc.BATCHES[name][-1]:
        ec = hc.edge_case(g, B, seed)
        for c in [ec] + [hc.variant(ec, g, v) for v in ('big_logits', 'gamma0', 'constant_plane')]:
            lo, hi = hc.margin(c, g)
            assert lo >= hc.MARGIN * hi
        assert (ec['w'] == 0).any() or B <= 2
        assert ec['w'][ec['w'] > 0].max() / ec['w'][ec['w'] > 0].min() > (1e2 if B > 3 else 1)
        assert B == 1 or (ec['idx'] != np.arange(B)).any()


def _looked_at(m, g):
    """What tests/test_gpu_heads.py compares, flat."""
    out = dict(loss=np.array([m['loss']]), prio=m['prio'], dF_pred=m['dF_pred'], dF_rew=m['dF_rew'], nbt=m['nbt'].astype(f64))
    for hd, hn in enumerate(hc.HEAD_NAMES):
        for k, v in m['grads'][hd].items():
            out[f'{hn}.d{k}'] = v
        out[f'{hn}.running_mean'], out[f'{hn}.running_var'] = m['running'][hd]
    for i, r in enumerate(m['groups']):
        out[f'g{i}.dlogit'] = r['loss']['dlogit']
        out[f'g{i}.c3'] = r['bnb']['c3']
    return out


# the geometry each mistake shows on (an even support for the spacing, a categorical head for the projection's constants)
MUT_GEOM = {'unit_spacing': 'atari_even', 'no_clamp': 'atari_odd', 'no_1e-5': 'atari_odd', 'priority_from_t1': 'atari_odd'}


@pytest.mark.parametrize('mut', hc.MUTATIONS)
def test_each_deliberate_mistake_moves_something_the_gpu_test_looks_at(mut):
    """The mistakes live in the numpy model only.  Each must move a compared tensor by more than 1e-6 of its largest element -- an order of magnitude
    above the float32 bars of the GPU test -- on the edge data."""
    g = HOST_GEOMS[MUT_GEOM.get(mut, 'board')]
    case = hc.edge_case(g, 6, 9)
    ref, bad = _looked_at(hc.model(case, g), g), _looked_at(hc.model(case, g, mut=mut), g)
    moved = {k: float(np.abs(np.asarray(bad[k], f64) - np.asarray(ref[k], f64)).max()) / max(1e-300, float(np.abs(ref[k]).max())) for k in ref}
    hit = {k: v for k, v in moved.items() if v > 1e-6}
    assert hit, f'{mut}: nothing moved (largest {max(moved.values()):.3g})'
    # and on an odd support the spacing mistake is no mistake
    if mut == 'unit_spacing':
        g2 = HOST_GEOMS['atari_odd']
        c2 = hc.edge_case(g2, 6, 9)
        _close(hc.model(c2, g2, mut=mut)['prio'], hc.model(c2, g2)['prio'], 'priorities at an odd support')
