"""games.BreakoutEnv (the specification of the device env MZ_ENV_BREAKOUT) and the numpy model of the device env (tests/breakout_cases.py),
without a GPU: scripted episodes for every rule branch with their states written out by hand and their frames compared byte for byte; the
model -- per-env state arrays, Philox start codes, restart, the flat 16-byte-run renderer -- equal to BreakoutEnv frame for frame on random
play over every shape; the condition that the smallest grid reaches every branch; nine planted mistakes, each seen by its named case."""
import re

import numpy as np
import pytest

import breakout_cases as bc
from helpers import REPO

G43 = bc.SHAPES['g43']


def _script_expected(name):
    cap, codes, moves = bc.SCRIPTS[name]
    shape = G43[:5] + (cap,)
    frames = [bc.paint(shape, *st) for _, _, _, st in moves]
    k = codes[0]
    first = bc.paint(shape, k >> 1, 2, 1, k >> 1, 2, ('###',))
    return shape, codes + [0] * 4, np.array([m[0] for m in moves]), np.array([m[1] for m in moves], np.float32), \
        np.array([m[2] for m in moves], np.uint8), np.stack([first] + frames)


def _play_script(name, where, bug=None):
    shape, codes, acts, _, _, _ = _script_expected(name)
    if where == 'host':
        return bc.play_host(bc.host_envs(1, shape, 0, codes=[codes]), acts[:, None])
    return bc.play_model(bc.BreakoutModel(1, *shape, codes=[codes], bug=bug), acts[:, None])


@pytest.mark.parametrize('where', ['host', 'model'])
@pytest.mark.parametrize('name', sorted(bc.SCRIPTS))
def test_scripted_episodes_match_the_hand_written_states(name, where):
    _, _, _, rewards, dones, frames = _script_expected(name)
    f, r, d = _play_script(name, where)
    assert r[:, 0].tobytes() == rewards.tobytes() and d[:, 0].tobytes() == dones.tobytes()
    assert f[:, 0].tobytes() == frames.tobytes()
    assert set(np.unique(frames)) <= {0, bc.BRICK, bc.TRAIL, bc.PADDLE, bc.BALL}


def test_scripts_cover_every_rule_branch():
    assert set(bc.SCRIPTS) == {'side_bounce', 'top_bounce', 'brick_hit', 'paddle_straight', 'paddle_corner', 'miss', 'refill', 'cap', 'cap_brick'}
    cap, _, moves = bc.SCRIPTS['cap_brick']
    assert moves[-1][1] == 1.0 and moves[-1][2] == 1 and len(moves) == cap  # a brick reward on the move the cap ends
    cap, _, moves = bc.SCRIPTS['cap']
    assert moves[-1][1] == 0.0 and moves[-1][2] == 1 and len(moves) == cap
    assert [m[2] for m in bc.SCRIPTS['miss'][2]] == [0, 0, 1, 1] and bc.SCRIPTS['miss'][0] > 4  # ended by misses, not by the cap
    assert bc.SCRIPTS['refill'][2][-2][3][5] == ('...',) and bc.SCRIPTS['refill'][2][-1][3][5] == ('###',)


def test_paint_priority_where_cells_coincide():
    from muzero_amd.games import BreakoutEnv

    env = BreakoutEnv(6, 5, 1, 1, brick_rows=2, start_codes=[0])
    env.reset()
    env.bx, env.by, env.lx, env.ly, env.px = 2, 5, 2, 5, 2  # ball, trail and paddle in one cell
    assert env.render()[0, 5, 2] == 255
    env.by = 4                                              # trail and paddle
    assert env.render()[0, 5, 2] == 160 and env.render()[0, 4, 2] == 255
    env.lx, env.ly = 1, 1                                   # trail on a brick
    assert env.render()[0, 1, 1] == 64 and env.render()[0, 1, 0] == 96 and env.render()[0, 0].sum() == 0
    env.bx, env.by = 1, 1                                   # ball on trail on brick
    assert env.render()[0, 1, 1] == 255


# (shape key, envs, moves): every grid and cell size of the issue; the atari shape plays few moves (the model paints byte by byte)
RANDOM_PLAY = [('g43', 8, 40), ('g43px', 8, 40), ('g65', 5, 60), ('g68', 3, 40), ('g32', 3, 60), ('atari', 2, 6)]


@pytest.mark.parametrize('key,B,moves', RANDOM_PLAY)
def test_model_equals_breakout_env_on_random_play(key, B, moves):
    shape = bc.SHAPES[key]
    acts = np.random.RandomState(5).randint(0, 3, size=(moves, B))
    fm, rm, dm = bc.play_model(bc.BreakoutModel(B, *shape, seed=11), acts)
    fh, rh, dh = bc.play_host(bc.host_envs(B, shape, 11), acts)
    assert fm.shape == (moves + 1, B, 1, shape[0] * shape[2], shape[1] * shape[3])
    assert fm.tobytes() == fh.tobytes() and rm.tobytes() == rh.tobytes() and dm.tobytes() == dh.tobytes()
    assert (fm == bc.BALL).any(axis=(2, 3, 4)).all() and (fm == bc.PADDLE).any(axis=(2, 3, 4)).all()


def test_shapes_hold_the_sizes_that_matter():
    cw = {k: v[3] for k, v in bc.SHAPES.items()}
    fe = {k: v[0] * v[2] * v[1] * v[3] for k, v in bc.SHAPES.items()}
    assert bc.SHAPES['g43'][:4] == (4, 3, 3, 4) and bc.SHAPES['g43px'][2:4] == (1, 1) and bc.SHAPES['atari'][2:4] == (8, 8)
    assert cw['g65'] % 4 and fe['g65'] % 16 and fe['g43px'] % 16  # a cell width no multiple of 4, frame sizes no multiple of 16
    assert bc.SHAPES['g32'][1] == 32 and bc.SHAPES['g32'][4] == 3 and bc.SHAPES['atari'][4:] == (3, 200)


def _branches(codes, actions, shape):
    """Counts of the rule branches games.BreakoutEnv takes on `actions` [moves, B] (host envs alone, restarted when done)."""
    from muzero_amd.games import BreakoutEnv

    rows, cols, ch, cw, K, cap = shape
    seen = dict(side=0, top=0, brick=0, straight=0, corner=0, miss=0, refill=0, cap=0, cap_brick=0)
    for e in range(actions.shape[1]):
        env = BreakoutEnv(rows, cols, 1, 1, brick_rows=K, max_moves=cap, start_codes=codes[e])
        env.reset()
        for a in actions[:, e]:
            bx, by, d, px0, bricks = env.bx, env.by, env.d, env.px, list(env.bricks)
            px = min(max(px0 + int(a) - 1, 0), cols - 1)
            nx, ny = bx + bc.DX[d], by + bc.DY[d]
            if not 0 <= nx < cols:
                seen['side'] += 1
                nx = min(max(nx, 0), cols - 1)
            _, r, done, _ = env.step(int(a))
            capped = env.t == cap
            if ny < 0:
                seen['top'] += 1
            elif r:
                seen['brick'] += 1
                seen['cap_brick'] += capped
            elif ny == rows - 1:
                seen['refill'] += not any(bricks)
                seen['straight' if bx == px else ('corner' if nx == px else 'miss')] += 1
            seen['cap'] += capped and not r
            if done:
                env.reset()
    return seen


def test_uniform_play_on_the_smallest_grid_reaches_every_branch():
    """8 envs x 40 moves of uniform play on the 4 x 3 grid with one brick row and cap 12: the run the GPU lock-step test replays."""
    shape = bc.SHAPES['g43']
    acts = np.random.RandomState(5).randint(0, 3, size=(40, 8))
    codes = [[bc.start_code(5, e, k, 3) for k in range(41)] for e in range(8)]
    seen = _branches(codes, acts, shape)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize('bug', bc.BUGS)
def test_planted_mistake_is_seen_by_its_named_case(bug):
    case = bc.SEEN_BY[bug]
    if case == 'wide32':  # the 32-column grid's first frame: the brick in column 31 of every row
        shape = bc.SHAPES['g32']
        good = bc.BreakoutModel(1, *shape, codes=[[0]]).frames()
        bad = bc.BreakoutModel(1, *shape, codes=[[0]], bug=bug).frames()
        assert (good[0, 0, 1:4, 31] == bc.BRICK).all() and good.tobytes() == bc.host_envs(1, shape, 0, codes=[[0]])[0].reset()[None].tobytes()
        assert good.tobytes() != bad.tobytes()
        return
    good, bad = _play_script(case, 'model'), _play_script(case, 'model', bug)
    assert any(g.tobytes() != b.tobytes() for g, b in zip(good, bad)), (bug, case)
    host = _play_script(case, 'host')
    assert all(g.tobytes() == h.tobytes() for g, h in zip(good, host))


def test_start_codes_and_wrappers():
    from muzero_amd import games, pipeline
    from muzero_amd.config import make_breakout_config

    # the package's own Philox helper draws what the tests' reference implementation draws
    for seed, e, k, cols in ((5, 0, 0, 3), (5, 7, 3, 12), (2 ** 40 + 9, 511, 1000, 32)):
        assert games.breakout_start_code(seed, e, k, cols) == bc.start_code(seed, e, k, cols)
    codes = [games.breakout_start_code(5, e, k, 12) for e in range(64) for k in range(8)]
    assert min(codes) >= 0 and max(codes) <= 23 and len(set(codes)) > 12
    env = games.BreakoutEnv(6, 5, 2, 3, brick_rows=2, max_moves=9, start_codes=[7])
    assert env.name == 'Breakout' and env.num_actions == 3 and env.observation_shape == (1, 12, 15) and env.max_episode_steps == 9
    env.reset()
    assert (env.bx, env.by, env.d, env.px, env.lx, env.ly) == (3, 3, 3, 2, 3, 3) and env.bricks == [31, 31]
    with pytest.raises(ValueError):
        env.reset(start_code=10)
    for bad in (dict(cols=33), dict(cols=2), dict(rows=5, brick_rows=3), dict(brick_rows=4), dict(brick_rows=0), dict(max_moves=0)):
        with pytest.raises(ValueError):
            games.BreakoutEnv(**bad)
    w = games.make_breakout_env(6, 5, 2, 3, stack_history=2, brick_rows=2, start_codes=[7, 7])
    obs = w.reset()
    assert obs.shape == (4, 12, 15) and obs.dtype == np.float32 and obs[0].max() == 1.0 and (obs[2:] == np.float32(1 / 3)).all()
    obs, r, d, _ = w.step(2)
    assert (obs[2] == np.float32(1.0)).all() and (obs[3] == np.float32(1 / 3)).all() and not d and w.name == 'Breakout'
    assert pipeline.device_stack_parts(w)[1:] == (2, True, True)
    assert 'Breakout' in pipeline.DEVICE_ENVS and 'Breakout' in pipeline.ARENA_ENVS
    assert pipeline.resolve_self_play_envs(w, 4) == ('device', 'Breakout') and pipeline.resolve_arena_env(env) == 'Breakout'
    assert pipeline._breakout_args(w) == dict(rows=6, cols=5, brick_rows=2, max_moves=200)
    cfg = make_breakout_config()
    assert cfg.input_shape == (8, 96, 96) and cfg.td_steps == 10 and cfg.discount < 1 and cfg.max_moves == 200 and cfg.num_actions == 3
    assert games.breakout_track_action(env) in (0, 1, 2)


def test_header_planner_and_kernel_header_agree():
    from muzero_amd import planner

    text = open(REPO + '/include/mzplanner.h').read()
    assert re.search(r'#define MZ_ENV_BREAKOUT 7\b', text) and planner.ENV_BREAKOUT == 7
    for name in ('mz_selfplay_reset_breakout', 'mz_arena_reset_breakout'):
        assert name in planner.ABI_SYMBOLS and re.search(r'\bint ' + name + r'\(', text)
    m = re.search(r'typedef struct \{([^}]*)\} mz_breakout_env;', text)
    fields = re.findall(r'(\w+)(?=[,;])', re.sub(r'/\*.*?\*/', '', m.group(1)))
    assert fields == [f for f, _ in planner.MzBreakoutEnv._fields_] == ['rows', 'cols', 'brick_rows', 'max_moves', 'record_format']
    hdr = open(REPO + '/muzero_amd/csrc/mz_breakout.h').read()
    assert 'BREAKOUT_STREAM = 0x%08xu' % bc.STREAM in hdr and 'ENV_BREAKOUT = 7' in hdr
    # the stream is free: no other header or test module keys a Philox stream with it
    catch = open(REPO + '/muzero_amd/csrc/mz_catch.h').read()
    assert '0x70000000u' in catch and '0x71000000' not in catch
