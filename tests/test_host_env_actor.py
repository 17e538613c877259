"""CPU side of self-play on host-stepped environments: how run_self_play routes `env` (device environment names and objects
unchanged; lists, factories and unknown env objects to the host-env loop), which envs get their frame stacking done on the device,
argument validation, and the C ABI declarations of the new entry points."""
import os
import re
import types

import numpy as np
import pytest

from helpers import REPO


def test_device_names_and_named_objects_keep_the_device_path():
    from muzero_amd import games, pipeline

    for name in pipeline.DEVICE_ENVS:
        assert pipeline.resolve_self_play_envs(name, 8) == ('device', name)
    assert pipeline.resolve_self_play_envs(games.TicTacToeEnv(), 8) == ('device', 'TicTacToe')
    assert pipeline.resolve_self_play_envs(games.GomokuEnv(board_size=9), 8) == ('device', 'Gomoku')
    spec_env = types.SimpleNamespace(spec=types.SimpleNamespace(id='CartPole-v1'), reset=lambda: 0, step=lambda a: 0)
    assert pipeline.resolve_self_play_envs(spec_env, 8) == ('device', 'CartPole-v1')
    with pytest.raises(ValueError, match="no device environment for 'Pong'"):
        pipeline.resolve_self_play_envs('Pong', 8)


def test_lists_factories_and_unknown_objects_go_to_the_host_loop():
    from muzero_amd import games, pipeline

    envs = [games.TicTacToeEnv() for _ in range(3)]
    kind, got = pipeline.resolve_self_play_envs(envs, 8)
    assert kind == 'host' and got == envs
    kind, got = pipeline.resolve_self_play_envs(tuple(envs), 8)
    assert kind == 'host' and got == envs
    calls = []

    def factory(i):
        calls.append(i)
        return games.CartPoleEnv(seed=i)

    kind, got = pipeline.resolve_self_play_envs(factory, 5)
    assert kind == 'host' and len(got) == 5 and calls == [0, 1, 2, 3, 4]
    one = games.CartPoleEnv()
    assert pipeline.resolve_self_play_envs(one, 8) == ('host', [one])  # no device env: B = 1


def test_routing_rejects_what_is_not_an_environment():
    from muzero_amd import pipeline

    for bad in (42, None, [], [object()]):
        with pytest.raises(ValueError):
            pipeline.resolve_self_play_envs(bad, 4)


def test_device_stacking_unwraps_the_reference_wrappers():
    from muzero_amd import games, pipeline

    cp = games.CartPoleEnv(stack_history=4)
    base, S, image, u8 = pipeline.device_stack_parts(cp)
    assert base is cp.env.env and (S, image, u8) == (4, False, False)

    class Frames:
        num_actions, observation_shape = 3, (1, 8, 8)

        def reset(self):
            return np.zeros((1, 8, 8), np.uint8)

        def step(self, a):
            return np.zeros((1, 8, 8), np.uint8), 0.0, False, {}

    raw = Frames()
    st = games.StackFrameAndAction(games.ScaledFloatFrame(raw), 2, is_obs_image=True)
    assert pipeline.device_stack_parts(st) == (raw, 2, True, True)
    st = games.StackFrameAndAction(raw, 3, is_obs_image=True)
    assert pipeline.device_stack_parts(games.PlayerIdAndActionMaskWrapper(st)) == (raw, 3, True, False)
    assert pipeline.device_stack_parts(games.TicTacToeEnv()) is None
    assert pipeline.device_stack_parts(raw) is None


def test_scaled_float_frame_is_numpy_float32_division():
    from muzero_amd import games

    class One:
        num_actions, observation_shape = 6, (1, 16, 16)

        def reset(self):
            return np.arange(256, dtype=np.uint8).reshape(1, 16, 16)

        def step(self, a):
            return self.reset(), 1.0, False, {}

    env = games.ScaledFloatFrame(One())
    x = env.reset()
    assert x.dtype == np.float32 and np.array_equal(x.reshape(-1), np.arange(256).astype(np.float32) / np.float32(255.0))
    # stacked on the host: the reference's observation layout, newest first, action planes (a + 1) / A
    st = games.StackFrameAndAction(games.ScaledFloatFrame(One()), 2, is_obs_image=True)
    st.reset()
    o = st.step(4)[0]
    assert o.shape == (4, 16, 16) and np.all(o[2] == np.float32(5 / 6)) and np.all(o[3] == np.float32(1 / 6))


def test_board_temperature_switch_reads_the_config_schedule():
    from muzero_amd import pipeline
    from muzero_amd.config import make_classic_config, make_gomoku_config, make_tictactoe_config

    assert pipeline.board_temperature_switch(make_tictactoe_config(use_tensorboard=False)) == 6
    assert pipeline.board_temperature_switch(make_gomoku_config(use_tensorboard=False)) == 30
    with pytest.raises(ValueError, match='1.0 for the first n moves'):
        pipeline.board_temperature_switch(make_classic_config(use_tensorboard=False))


def test_env_threads_are_bounded_before_any_gpu_work():
    from muzero_amd import games, pipeline

    cfg = types.SimpleNamespace(num_envs=2, is_board_game=False)
    for n in (0, 17):
        with pytest.raises(ValueError, match='env_threads must be 1 to 16'):
            pipeline.run_self_play(cfg, 0, None, None, [games.CartPoleEnv(), games.CartPoleEnv()], None, None, None, env_threads=n)


def test_header_declares_the_external_env_abi():
    from muzero_amd import planner

    text = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    assert re.search(r'#define MZ_ENV_EXTERNAL 5\b', text) and planner.ENV_EXTERNAL == 5
    for name in ('mz_selfplay_reset_external', 'mz_selfplay_external_act', 'mz_selfplay_external_commit'):
        assert name in planner.ABI_SYMBOLS and re.search(r'\bint ' + name + r'\(', text)
    end = text.index('} mz_external_env;')
    body = text[text.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(\w+)\s*[,;]', body)
    assert fields == [f for f, _ in planner.MzExternalEnv._fields_]


def test_build_keeps_ieee_division():
    """k_ext_ingest's uint8 / 255.0f must be the correctly rounded float32 division numpy does (ScaledFloatFrame)."""
    from muzero_amd import build

    flags = ' '.join(build.FLAGS)
    for bad in ('-ffast-math', '-fno-hip-fp32-correctly-rounded-divide-sqrt', '-funsafe-math-optimizations', '-freciprocal-math'):
        assert bad not in flags
