"""Reloading planner weights from device memory (mz_planner_bind_param_device / mz_planner_refresh_params): what can be checked without a
GPU -- the two entry points are declared, listed and exported, and the pure validation of a state_dict names what it cannot bind."""
import ctypes
import os
import re

import pytest
import torch

from helpers import REPO, build_mlp, mlp_case

ENTRIES = ('mz_planner_bind_param_device', 'mz_planner_refresh_params')


def test_entry_points_are_declared_listed_and_exported():
    from muzero_amd import build, planner

    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mzplanner.h')).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/mzplanner.h'
        assert name in planner.ABI_SYMBOLS
        assert hasattr(lib, name), f'{name} is not exported'
    for hook in ('mz_debug_read_packed', 'mz_debug_packed_info', 'mz_debug_conv3x3'):  # test hooks: exported, not part of the header
        assert hasattr(lib, hook) and hook not in text


def test_header_documents_the_entries_with_the_reference_hand_off():
    text = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    block = text[text.index('Weights that already live on the planner'):text.index('int mz_planner_refresh_params')]
    assert 'pipeline.py:266' in block and 'MZ_E_STATE' in block and 'MZ_E_INVALID' in block


class _FakeCuda:
    """A tensor stand-in that claims to live on a GPU (device_weights only reads attributes: no GPU is touched)."""

    def __init__(self, t, index=0):
        self._t, self.device, self.dtype = t, torch.device('cuda', index), t.dtype

    def is_contiguous(self):
        return self._t.is_contiguous()

    def detach(self):
        return self


def test_validation_rejects_what_cannot_be_bound_by_name(monkeypatch):
    from muzero_amd import planner

    sd = build_mlp(mlp_case('tiny')).state_dict()
    key = 'dynamics_net.transition_net.0.weight'
    with pytest.raises(ValueError, match=re.escape(next(iter(sd)))):  # CPU tensors: the first key is named
        planner.device_weights(sd, 0)
    assert not planner.can_bind(sd, 0)

    monkeypatch.setattr(planner, '_is_tensor', lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))
    on_gpu = {k: _FakeCuda(v) for k, v in sd.items()}
    assert set(planner.device_weights(on_gpu, 0)) == set(sd)
    assert planner.can_bind(on_gpu, 0)

    bad = dict(on_gpu)
    bad[key] = sd[key]  # one CPU tensor among GPU tensors
    with pytest.raises(ValueError, match=re.escape(key)):
        planner.device_weights(bad, 0)
    bad[key] = _FakeCuda(sd[key].double())
    with pytest.raises(ValueError, match=re.escape(key) + '.*float64'):
        planner.device_weights(bad, 0)
    bad[key] = _FakeCuda(sd[key].t())
    assert not sd[key].t().is_contiguous()
    with pytest.raises(ValueError, match=re.escape(key) + '.*contiguous'):
        planner.device_weights(bad, 0)
    bad[key] = _FakeCuda(sd[key], index=1)  # another GPU
    with pytest.raises(ValueError, match=re.escape(key)):
        planner.device_weights(bad, 0)
    missing = {k: v for k, v in on_gpu.items() if k != key}
    with pytest.raises(ValueError, match=re.escape(key)):
        planner.device_weights(missing, 0, expect=sd.keys())


def test_num_batches_tracked_is_skipped():
    from muzero_amd import planner

    sd = {'bn.running_mean': _FakeCuda(torch.zeros(3)), 'bn.num_batches_tracked': torch.tensor(7)}
    import unittest.mock as mock

    with mock.patch.object(planner, '_is_tensor', lambda t: True):
        assert list(planner.device_weights(sd, 0)) == ['bn.running_mean']
