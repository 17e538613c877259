"""Host side of the image arena without a GPU: the numpy model of tests/arena_image_cases.py against games.make_catch_env objects byte for
byte, each planted mistake seen by its named case, pipeline.play_match's Catch front end up to the planner, and the new kernels'
cross-compiled resource usage."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import arena_image_cases as ac
from helpers import build_mlp

B = 12  # >= rows - 1 of every shape: start rows 0 and rows - 2 in one batch
FIELDS = ('root', 'live', 'length', 'ret', 'draws', 'finished_plies', 'n_live')


def _case(shape, S, name, bug=None):
    rows, cols, ch, cw = ac.SHAPES[shape]
    bc, sr = ac.layout(B, rows, cols)
    assert sr.min() == 0 and sr.max() == rows - 2
    actions = ac.script(name, B, rows + 1)  # two plies past the longest game: frozen envs are stepped over
    got = ac.play_model(ac.ImageArenaModel(rows, cols, ch, cw, S, bc, sr, bug), actions)
    return got, (rows, cols, ch, cw, bc, sr, actions)


@pytest.mark.parametrize('S', ac.STACKS)
@pytest.mark.parametrize('shape', sorted(ac.SHAPES))
def test_model_equals_host_catch_envs(shape, S):
    """Roots byte for byte, live flags, lengths, returns and the tally at every ply, for every script."""
    for name in ac.SCRIPTS:
        got, (rows, cols, ch, cw, bc, sr, actions) = _case(shape, S, name)
        want = ac.play_host(ac.host_envs(rows, cols, ch, cw, S, bc, sr), actions)
        for k in FIELDS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (shape, S, name, k)
        assert got['n_live'][-1] == 0 and got['draws'][-1] == B
        np.testing.assert_array_equal(got['length'][-1], rows - 1 - sr)
        assert set(np.unique(got['ret'][-1])) <= {-1.0, 1.0}
        # the first ply: every frame plane is the first frame, every action plane holds action 0
        r0 = got['root'][0]
        assert all((r0[:, k] == r0[:, 0]).all() for k in range(S)) and (r0[:, S:] == ac.action_value(0)).all()


@pytest.mark.parametrize('bug', ac.BUGS)
def test_planted_mistake_is_seen_by_its_named_case(bug):
    shape, S, name = ac.SEEN_BY[bug]
    clean, _ = _case(shape, S, name)
    bad, _ = _case(shape, S, name, bug)
    assert any(clean[k].tobytes() != bad[k].tobytes() for k in FIELDS), bug


def test_pipeline_resolves_catch_and_refuses_opponents_before_any_planner():
    from muzero_amd import pipeline
    from muzero_amd.config import make_atari_config
    from muzero_amd.games import CatchEnv, make_catch_env

    assert 'Catch' in pipeline.ARENA_ENVS
    assert pipeline.resolve_arena_env('Catch') == 'Catch'
    assert pipeline.resolve_arena_env(CatchEnv(6, 4, 2, 3)) == 'Catch'
    assert pipeline.resolve_arena_env(make_catch_env(12, 12, 1, 1, stack_history=2)) == 'Catch'
    with pytest.raises(ValueError):
        pipeline.resolve_arena_env('Synthetic-Atari')
    net = build_mlp(('c1s2', (4, 12, 12), 3, 32, 7, 5, 16, 41))
    cfg = make_atari_config(use_tensorboard=False)
    dev = types.SimpleNamespace(index=0)
    envs = [make_catch_env(12, 12, 1, 1, stack_history=2) for _ in range(4)]
    for env, opponent in (('Catch', net), ('Catch', 'random'), (CatchEnv(), net), (envs, net), (envs, 'random'), (lambda i: envs[i], 'random')):
        with pytest.raises(ValueError):
            pipeline.play_match(cfg, net, opponent, dev, env, 4)
    with pytest.raises(ValueError):
        pipeline.play_match(cfg, net, None, dev, 'Catch', 0)
    with pytest.raises(ValueError):
        pipeline.play_match(cfg, net, None, dev, 'Catch', 4, init_state=np.zeros((4, 4)))
    with pytest.raises(ValueError):
        pipeline.play_match(cfg, net, None, dev, 'Synthetic-Atari', 4)
    with pytest.raises(ValueError):
        pipeline.play_match(cfg, net, None, dev, envs, 5)  # four env objects for five games


def test_image_arena_kernels_cross_compile_without_scratch_spills_or_lds(tmp_path):
    """mz_arena_image.h and the two game headers on it (mz_catch.h, mz_breakout.h), device side, for gfx950 with the library's flags: the
    arena's kernels (both forms of the root builder) and every instance of mz_grid_game.h's four kernel templates for both games are there,
    and the compiler reports no scratch memory, no register spills and no LDS for them."""
    from muzero_amd import build

    hipcc = os.environ.get('HIPCC', 'hipcc')
    if shutil.which(hipcc) is None:
        pytest.fail('hipcc not found: the image arena kernels cannot be compiled')
    games, templates = ('Catch', 'Breakout'), ('k_game_reset', 'k_game_step', 'k_game_render', 'k_game_arena_step')
    src = tmp_path / 'arena_image_tu.hip'
    src.write_text('#include "mz_catch.h"\n#include "mz_breakout.h"\n'
                   'template __global__ void mz::k_imgarena_ingest<4>(const mz::ImgArenaLaunch);\n'
                   'template __global__ void mz::k_imgarena_ingest<1>(const mz::ImgArenaLaunch);\n' +
                   ''.join(f'template __global__ void mz::{t}<mz::{g}>(const mz::GameLaunch<mz::{g}>);\n' for g in games for t in templates[:3]) +
                   ''.join(f'template __global__ void mz::k_game_arena_step<mz::{g}>(const mz::ImgArenaLaunch, const mz::{g});\n' for g in games))
    flags = [f for f in build.FLAGS if f not in ('-shared', '-fPIC')]
    out = subprocess.run([hipcc] + flags + ['--cuda-device-only', '-c', '-Rpass-analysis=kernel-resource-usage', '-I', build.CSRC, str(src), '-o',
                                            str(tmp_path / 'arena_image_tu.o')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for b in re.split(r'remark: Function Name: ', out.stderr)[1:]:
        m = re.match(r'\S*?(k_imgarena_[a-z_]+?)(ILi(\d)EEE\S*|E\S*)\s', b)
        t = re.match(r'\S*?(k_game_[a-z_]+?)INS_\d+([A-Za-z]+)EEE\S*\s', b)  # a template instance is named with its argument
        if m or t:
            name = m.group(1) + (f'<{m.group(3)}>' if m.group(3) else '') if m else f'{t.group(1)}<{t.group(2)}>'
            found[name] = {k: int(v) for k, v in re.findall(r'remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)', b)}
    assert sorted(found) == sorted(['k_imgarena_commit', 'k_imgarena_ingest<1>', 'k_imgarena_ingest<4>', 'k_imgarena_record', 'k_imgarena_reset'] +
                                   [f'{t}<{g}>' for g in games for t in templates])
    for name, use in found.items():
        assert use['ScratchSize'] == 0 and use['SGPRs Spill'] == 0 and use['VGPRs Spill'] == 0, (name, use)
        assert use['LDS Size'] == 0 and use['VGPRs'] <= 128, (name, use)
    # mz_arena.h stays a translation unit of its own: it does not pull the image arena in
    with open(os.path.join(build.CSRC, 'mz_arena.h')) as f:
        assert 'mz_arena_image.h' not in f.read()
    # and the arena header knows no game: the game headers include it, not the other way round
    with open(os.path.join(build.CSRC, 'mz_arena_image.h')) as f:
        assert '#include "mz_catch.h"' not in f.read()
