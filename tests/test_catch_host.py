"""games.CatchEnv -- the specification of the device env MZ_ENV_CATCH -- on scripted episodes; the exact value of the random policy; the
numpy model of the device env (tests/catch_cases.py) against CatchEnv step for step, with every planted mistake seen by its named case; the
ABI text and the pipeline's routing.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

import catch_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, B, MOVES = 5, 8, 40


def paint(rows, cols, ch, cw, br, bc, pc):
    f = np.zeros((1, rows * ch, cols * cw), np.uint8)
    for y in range(rows * ch):
        for x in range(cols * cw):
            if (y // ch == br and x // cw == bc) or (y // ch == rows - 1 and x // cw == pc):
                f[0, y, x] = 255
    return f


def test_rules_on_scripted_episodes():
    from muzero_amd.games import CatchEnv

    env = CatchEnv(6, 5, 1, 1)
    assert env.name == 'Catch' and env.num_actions == 3 and env.observation_shape == (1, 6, 5) and env.max_episode_steps == 5
    # wall clipping, left: the paddle starts at column 2 and stops at 0
    env.reset(ball_col=0)
    seen = []
    for t in range(5):
        _, r, d, _ = env.step(0)
        seen.append((env.pc, r, d))
    assert seen == [(1, 0.0, False), (0, 0.0, False), (0, 0.0, False), (0, 0.0, False), (0, 1.0, True)]  # done exactly on the fifth move
    with pytest.raises(RuntimeError):
        env.step(1)
    # right: stops at cols - 1; the ball in column 0 is missed
    env.reset(ball_col=0)
    seen = [env.step(2)[1:3] + (env.pc,) for _ in range(5)]
    assert [s[2] for s in seen] == [3, 4, 4, 4, 4] and seen[-1][:2] == (-1.0, True) and all(s[:2] == (0.0, False) for s in seen[:-1])
    # the paddle moves BEFORE the catch test: one column off, the last move catches
    env.reset(ball_col=3)
    for _ in range(4):
        env.step(1)
    frame, r, d, _ = env.step(2)
    assert (r, d) == (1.0, True) and (env.br, env.bc, env.pc) == (5, 3, 3)
    assert frame.sum() == 255 and frame[0, 5, 3] == 255  # ball and paddle meet in one cell
    # start_row = rows - 2: an episode of one move
    one = CatchEnv(6, 5, 1, 1, start_row=4)
    one.reset(ball_col=2)
    assert one.step(1)[1:3] == (1.0, True)
    one.reset(ball_col=2)
    assert one.step(0)[1:3] == (-1.0, True)
    with pytest.raises(ValueError):
        env.reset(ball_col=5)
    with pytest.raises(ValueError):
        CatchEnv(6, 5, 1, 1, start_row=5)
    # the env's own draws cover the columns; first_row holds for the first episode only
    own = CatchEnv(6, 5, 1, 1, seed=3, first_row=3)
    own.reset()
    assert own.br == 3
    cols = set()
    for _ in range(60):
        own.reset()
        assert own.br == 0
        cols.add(own.bc)
    assert cols == set(range(5))


@pytest.mark.parametrize('shape', list(cc.SHAPES))
def test_frames_are_a_direct_paint(shape):
    from muzero_amd.games import CatchEnv

    rows, cols, ch, cw = cc.SHAPES[shape]
    env = CatchEnv(rows, cols, ch, cw)
    rs = np.random.RandomState(2)
    n = 0
    for bc in (0, cols - 1, cols // 2, 1):
        frame = env.reset(ball_col=bc)
        done = False
        while True:
            assert frame.dtype == np.uint8 and frame.tobytes() == paint(rows, cols, ch, cw, env.br, env.bc, env.pc).tobytes()
            n += 1
            if done:
                break
            frame, _, done, _ = env.step(int(rs.randint(3)))
    assert n == 4 * rows


@pytest.mark.parametrize('S', [1, 2, 4])
def test_stacked_observation(S):
    from muzero_amd import games

    env = games.make_catch_env(6, 4, 2, 3, stack_history=S)
    assert isinstance(env, games.PlayerIdAndActionMaskWrapper) and env.name == 'Catch' and env.num_actions == 3
    assert env.current_player == env.opponent_player == 1 and env.actions_mask.tolist() == [True] * 3
    obs = env.reset(ball_col=1)
    assert obs.shape == (2 * S, 12, 12) == env.observation_shape and obs.dtype == np.float32
    first = paint(6, 4, 2, 3, 0, 1, 2).astype(np.float32) / 255.0
    for k in range(S):
        assert obs[k].tobytes() == first[0].tobytes()
        assert (obs[S + k] == np.float32(1 / 3)).all()  # action 0: (0 + 1) / 3
    obs, r, d, _ = env.step(2)
    assert obs[0].tobytes() == (paint(6, 4, 2, 3, 1, 1, 3).astype(np.float32) / 255.0)[0].tobytes()
    assert (obs[S] == np.float32(1.0)).all() and (r, d) == (0.0, False)  # (2 + 1) / 3
    if S > 1:
        assert obs[1].tobytes() == first[0].tobytes() and (obs[S + 1] == np.float32(1 / 3)).all()
    same = games.StackFrameAndAction(games.ScaledFloatFrame(games.CatchEnv(6, 4, 2, 3)), S, True)
    assert same.reset(ball_col=1).tobytes() == env.reset(ball_col=1).tobytes()


def test_random_policy_value():
    from muzero_amd.games import CatchEnv, catch_random_policy_return

    # exact: every one of the 3^(rows - 1) action strings, every ball column
    rows = cols = 5
    total = 0.0
    for bc in range(cols):
        for acts in itertools.product(range(3), repeat=rows - 1):
            env = CatchEnv(rows, cols, 1, 1)
            env.reset(ball_col=bc)
            for a in acts:
                _, r, _, _ = env.step(a)
            total += r
    brute = total / (cols * 3 ** (rows - 1))
    assert abs(catch_random_policy_return(rows, cols) - brute) < 1e-12
    # Monte Carlo at 12 x 12: returns are +-1, so the standard error comes from the sample itself
    env, rs, n = CatchEnv(12, 12, 1, 1, seed=7), np.random.RandomState(8), 20000
    rets = np.empty(n)
    for i in range(n):
        env.reset()
        done = False
        while not done:
            _, r, done, _ = env.step(int(rs.randint(3)))
        rets[i] = r
    v = catch_random_policy_return(12, 12)
    assert -1.0 < v < 0.0
    assert abs(rets.mean() - v) < 3 * rets.std(ddof=1) / np.sqrt(n), (rets.mean(), v)
    assert abs(catch_random_policy_return(12, 12, start_row=10) - (-1 + 2 * 3 / 36)) < 1e-12  # one move: 3 of 12 columns reachable, each by 1 action of 3


@pytest.mark.parametrize('shape', list(cc.SHAPES))
def test_model_is_the_host_env(shape):
    rows, cols, ch, cw = cc.SHAPES[shape]
    for name in cc.SCRIPTS:
        acts = cc.script(name, B, rows, cols, SEED, MOVES)
        fm, rm, dm = cc.play_model(cc.CatchModel(B, rows, cols, ch, cw, SEED), acts)
        fh, rh, dh = cc.play_host(cc.host_envs(B, rows, cols, ch, cw, SEED), acts)
        assert fm.tobytes() == fh.tobytes() and rm.tobytes() == rh.tobytes() and dm.tobytes() == dh.tobytes(), name
        assert dm.sum() >= 3 * B  # at least three episodes per env
        # the stagger: env e's first episode ends after rows - 1 - e % (rows - 1) moves, the later ones every rows - 1
        for e in range(B):
            ends = np.flatnonzero(dm[:, e])
            assert ends[0] == rows - 2 - e % (rows - 1) and (np.diff(ends) == rows - 1).all()
    # the cases cover what they are named for
    _, r, _ = cc.play_model(cc.CatchModel(B, rows, cols, ch, cw, SEED), cc.script('last_move', B, rows, cols, SEED, MOVES))
    assert (r > 0).any() and (r < 0).any()
    assert len({cc.ball_col(SEED, e, k, cols) for e in range(B) for k in range(4)}) > 2


@pytest.mark.parametrize('bug', cc.BUGS)
def test_each_planted_mistake_changes_its_case(bug):
    rows, cols, ch, cw = cc.SHAPES['c1']
    acts = cc.script(cc.SEEN_BY[bug], B, rows, cols, SEED, MOVES)
    good = cc.play_model(cc.CatchModel(B, rows, cols, ch, cw, SEED), acts)
    bad = cc.play_model(cc.CatchModel(B, rows, cols, ch, cw, SEED, bug=bug), acts)
    assert any(g.tobytes() != b.tobytes() for g, b in zip(good, bad)), bug


def test_abi_text_and_routing():
    from muzero_amd import games, pipeline, planner

    text = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    assert re.search(r'#define MZ_ENV_CATCH 6\b', text) and planner.ENV_CATCH == 6
    body = re.search(r'typedef struct \{([^}]*)\} mz_catch_env;', text)
    assert body and re.findall(r'int32_t ([a-z_, ]+);', re.sub(r'/\*.*?\*/', '', body.group(1), flags=re.S)) == ['rows, cols', 'record_format']
    assert re.search(r'int mz_selfplay_reset_catch\(mz_planner\* p, const mz_catch_env\* env\);', text)
    assert [f[0] for f in planner.MzCatchEnv._fields_] == ['rows', 'cols', 'record_format']
    assert 'Catch' in pipeline.DEVICE_ENVS
    assert pipeline.resolve_self_play_envs('Catch', 8) == ('device', 'Catch')
    assert pipeline.resolve_self_play_envs(games.CatchEnv(), 8) == ('device', 'Catch')
    assert pipeline.resolve_self_play_envs(games.make_catch_env(), 8) == ('device', 'Catch')
    kind, envs = pipeline.resolve_self_play_envs([games.make_catch_env() for _ in range(3)], 8)
    assert kind == 'host' and len(envs) == 3
    kind, envs = pipeline.resolve_self_play_envs(lambda i: games.CatchEnv(seed=i), 4)
    assert kind == 'host' and len(envs) == 4
    assert pipeline.device_stack_parts(games.make_catch_env(stack_history=2))[1:] == (2, True, True)


def test_catch_config():
    from muzero_amd.config import make_catch_config

    cfg = make_catch_config()
    assert cfg.num_actions == 3 and cfg.input_shape == (8, 96, 96) and not cfg.is_board_game
    assert cfg.value_support_size > 1 and cfg.reward_support_size > 1  # categorical heads
    assert cfg.acc_seq_length + cfg.unroll_steps + cfg.td_steps > cfg.rows - 1 and cfg.td_steps >= cfg.rows - 1
    assert cfg.visit_softmax_temperature_fn(0, 0) == 1.0
