"""Scripted Othello games with the board written out after every ply, and a numpy model of the device step (csrc/mz_othello.h).

Shapes, the smallest at which each thing can still go wrong:
  S  4 x 4, 18 actions: one lane per point; reaches a pass, an early end, a draw and a wipe-out within a dozen plies;
  N  4 x 6, 26 actions: not square (shifts by cols - 1 = 5 and cols + 1 = 7 are not shifts by rows +- 1), more than a 16-lane group;
  M  6 x 6, 38 actions: the example's board;
  F  8 x 8, 66 actions: the game itself, all 64 bits of the bitboard.
A case: `moves` (action per ply, black first: a point r * cols + c, rows * cols passes, rows * cols + 1 resigns), `boards` the position
after EVERY ply (rows top to bottom, '.' empty, 'X' black, 'O' white), `reward` / `done` of the last move and `winner` (1 black, 2 white,
None).  Every earlier move has reward 0 and done False.  The move lists were found by searching uniformly random games for the shortest
one with the property the case is named after, and the boards are the positions `games.OthelloEnv` reached on those lists, printed and
read through: they are NOT independent of the implementation.  What holds them to the rules independently is in
tests/test_othello_host.py: code that looks at the boards alone (`flipped_by_direction`, `ray`) checks what each case's name claims and
re-derives every ply's legal placements from the rays, and the env itself is held to the published perft counts.

`OthModel` is the kernel's formulation in numpy / Python integers: one byte per point, the two colours' bitboards (bit = point) rebuilt
from the bytes, a direction as a masked shift (by 1, cols - 1, cols, cols + 1, left or right; the mask clears the column the shift wraps
into and everything past bit nn), the flips of the chosen point and both colours' legal placements by directional flood fills of at most
max(rows, cols) - 2 steps, the end test and the count, both histories shifted, the next side's observation, the rebuilt mask, the
auto-reset.  `bug` plants one mistake."""
import numpy as np

SHAPES = {'S': (4, 4), 'N': (4, 6), 'M': (6, 6), 'F': (8, 8)}
# (dr, dc) of direction d, in the kernel's order: shifts by +1, +(cols - 1), +cols, +(cols + 1), then their opposites
DIRECTIONS = ((0, 1), (1, -1), (1, 0), (1, 1), (0, -1), (-1, 1), (-1, 0), (-1, -1))
DIRECTION_NAMES = ('east', 'south_west', 'south', 'south_east', 'west', 'north_east', 'north', 'north_west')


def _case(name, shape, moves, boards, reward=0.0, done=False, winner=None):
    return dict(name=name, shape=shape, moves=moves, boards=boards, reward=reward, done=done, winner=winner)


CASES = [
    # ---- S: 4 x 4 ----
    _case('draw', 'S', [14, 7, 3, 13, 4, 15, 11, 1, 12, 2, 0, 8],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OOO', '.XX.', '..X.'], ['...X', '.OXO', '.XX.', '..X.'], ['...X', '.OXO', '.OO.', '.OX.'], ['...X', 'XXXO', '.XO.', '.OX.'], ['...X', 'XXXO', '.XO.', '.OOO'], ['...X', 'XXXX', '.XXX', '.OOO'], ['.O.X', 'XOXX', '.OXX', '.OOO'], ['.O.X', 'XOXX', '.XXX', 'XOOO'], ['.OOX', 'XOOX', '.XOX', 'XOOO'], ['XXXX', 'XOOX', '.XOX', 'XOOO'], ['XXXX', 'XOOX', 'OOOX', 'XOOO']], 0.0, True, None),
    _case('edge_run_without_anchor', 'S', [1, 8, 13],
          [['.X..', '.XX.', '.XO.', '....'], ['.X..', '.XX.', 'OOO.', '....'], ['.X..', '.XX.', 'OXO.', '.X..']]),
    _case('end_full_board', 'S', [14, 15, 1, 8, 4, 0, 11, 7, 3, 13, 12, 2],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OX.', '.XO.', '..XO'], ['.X..', '.XX.', '.XO.', '..XO'], ['.X..', '.XX.', 'OOO.', '..XO'], ['.X..', 'XXX.', 'OXO.', '..XO'], ['OX..', 'OOX.', 'OXO.', '..XO'], ['OX..', 'OOX.', 'OXXX', '..XO'], ['OX..', 'OOOO', 'OXXO', '..XO'], ['OX.X', 'OOXO', 'OXXO', '..XO'], ['OX.X', 'OOXO', 'OOOO', '.OOO'], ['OX.X', 'OOXO', 'OXOO', 'XOOO'], ['OOOX', 'OOOO', 'OXOO', 'XOOO']], 1.0, True, 2),
    _case('end_with_empty_cells', 'S', [4, 8, 12, 0, 2, 16, 15],
          [['....', 'XXX.', '.XO.', '....'], ['....', 'XXX.', 'OOO.', '....'], ['....', 'XXX.', 'XXO.', 'X...'], ['O...', 'XOX.', 'XXO.', 'X...'], ['O.X.', 'XXX.', 'XXO.', 'X...'], ['O.X.', 'XXX.', 'XXO.', 'X...'], ['O.X.', 'XXX.', 'XXX.', 'X..X']], 1.0, True, 1),
    _case('final_placement_loses', 'S', [1, 2, 7, 0, 4, 8, 13, 14, 15],
          [['.X..', '.XX.', '.XO.', '....'], ['.XO.', '.XO.', '.XO.', '....'], ['.XO.', '.XXX', '.XO.', '....'], ['OOO.', '.OXX', '.XO.', '....'], ['OOO.', 'XXXX', '.XO.', '....'], ['OOO.', 'OOXX', 'OOO.', '....'], ['OOO.', 'OOXX', 'OOX.', '.X..'], ['OOO.', 'OOOX', 'OOO.', '.XO.'], ['OOO.', 'OOOX', 'OOO.', '.XXX']], -1.0, True, 2),
    _case('flip_east', 'S', [4],
          [['....', 'XXX.', '.XO.', '....']]),
    _case('flip_north', 'S', [14],
          [['....', '.OX.', '.XX.', '..X.']]),
    _case('flip_north_east', 'S', [1, 8, 12],
          [['.X..', '.XX.', '.XO.', '....'], ['.X..', '.XX.', 'OOO.', '....'], ['.X..', '.XX.', 'OXO.', 'X...']]),
    _case('flip_north_west', 'S', [14, 15],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OX.', '.XO.', '..XO']]),
    _case('flip_south', 'S', [1],
          [['.X..', '.XX.', '.XO.', '....']]),
    _case('flip_south_east', 'S', [1, 0],
          [['.X..', '.XX.', '.XO.', '....'], ['OX..', '.OX.', '.XO.', '....']]),
    _case('flip_south_west', 'S', [14, 7, 3],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OOO', '.XX.', '..X.'], ['...X', '.OXO', '.XX.', '..X.']]),
    _case('flip_three_directions', 'S', [1, 8, 13, 0, 4, 2],
          [['.X..', '.XX.', '.XO.', '....'], ['.X..', '.XX.', 'OOO.', '....'], ['.X..', '.XX.', 'OXO.', '.X..'], ['OX..', '.OX.', 'OXO.', '.X..'], ['OX..', 'XXX.', 'OXO.', '.X..'], ['OOO.', 'XOO.', 'OXO.', '.X..']]),
    _case('flip_west', 'S', [11],
          [['....', '.OX.', '.XXX', '....']]),
    _case('flipped_twice', 'S', [14, 15],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OX.', '.XO.', '..XO']]),
    _case('forced_pass', 'S', [1, 2, 11, 0, 16],
          [['.X..', '.XX.', '.XO.', '....'], ['.XO.', '.XO.', '.XO.', '....'], ['.XO.', '.XX.', '.XXX', '....'], ['OOO.', '.XX.', '.XXX', '....'], ['OOO.', '.XX.', '.XXX', '....']]),
    _case('run_broken_by_empty', 'S', [4, 2, 11, 12, 1, 0],
          [['....', 'XXX.', '.XO.', '....'], ['..O.', 'XXO.', '.XO.', '....'], ['..O.', 'XXO.', '.XXX', '....'], ['..O.', 'XXO.', '.OXX', 'O...'], ['.XO.', 'XXX.', '.OXX', 'O...'], ['OOO.', 'XXX.', '.OXX', 'O...']]),
    _case('two_passes_same_side', 'S', [1, 8, 15, 2, 3, 11, 0, 16, 7, 16],
          [['.X..', '.XX.', '.XO.', '....'], ['.X..', '.XX.', 'OOO.', '....'], ['.X..', '.XX.', 'OOX.', '...X'], ['.XO.', '.OX.', 'OOX.', '...X'], ['.XXX', '.OX.', 'OOX.', '...X'], ['.XXX', '.OX.', 'OOOO', '...X'], ['XXXX', '.XX.', 'OOXO', '...X'], ['XXXX', '.XX.', 'OOXO', '...X'], ['XXXX', '.XXX', 'OOXX', '...X'], ['XXXX', '.XXX', 'OOXX', '...X']]),
    _case('wipe_out', 'S', [14, 15, 4, 8, 13, 12, 11, 7, 16, 1, 16, 0],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OX.', '.XO.', '..XO'], ['....', 'XXX.', '.XO.', '..XO'], ['....', 'XXX.', 'OOO.', '..XO'], ['....', 'XXX.', 'OXO.', '.XXO'], ['....', 'XXX.', 'OXO.', 'OOOO'], ['....', 'XXX.', 'OXXX', 'OOOO'], ['....', 'XXXO', 'OXOO', 'OOOO'], ['....', 'XXXO', 'OXOO', 'OOOO'], ['.O..', 'XOOO', 'OOOO', 'OOOO'], ['.O..', 'XOOO', 'OOOO', 'OOOO'], ['OO..', 'OOOO', 'OOOO', 'OOOO']], 1.0, True, 2),
    _case('wrap_east', 'S', [11, 13, 4],
          [['....', '.OX.', '.XXX', '....'], ['....', '.OX.', '.OXX', '.O..'], ['....', 'XXX.', '.OXX', '.O..']]),
    _case('wrap_north_east', 'S', [14, 7],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OOO', '.XX.', '..X.']]),
    _case('wrap_north_west', 'S', [14, 13, 8],
          [['....', '.OX.', '.XX.', '..X.'], ['....', '.OX.', '.OX.', '.OX.'], ['....', '.OX.', 'XXX.', '.OX.']]),
    _case('wrap_south_east', 'S', [1, 2, 7],
          [['.X..', '.XX.', '.XO.', '....'], ['.XO.', '.XO.', '.XO.', '....'], ['.XO.', '.XXX', '.XO.', '....']]),
    _case('wrap_south_west', 'S', [1, 8],
          [['.X..', '.XX.', '.XO.', '....'], ['.X..', '.XX.', 'OOO.', '....']]),
    _case('wrap_west', 'S', [4, 8, 12],
          [['....', 'XXX.', '.XO.', '....'], ['....', 'XXX.', 'OOO.', '....'], ['....', 'XXX.', 'XXO.', 'X...']]),
    _case('resign_black', 'S', [17], [['....', '.OX.', '.XO.', '....']], -1.0, True, 2),
    _case('resign_white', 'S', [1, 17], [['.X..', '.XX.', '.XO.', '....'], ['.X..', '.XX.', '.XO.', '....']], -1.0, True, 1),
    # ---- N: 4 x 6 ----
    _case('draw', 'N', [2, 3, 10, 1, 20, 21, 22, 5, 16, 23, 4, 19, 0, 7, 6, 17],
          [['..X...', '..XX..', '..XO..', '......'], ['..XO..', '..XO..', '..XO..', '......'], ['..XO..', '..XXX.', '..XO..', '......'], ['.OOO..', '..OXX.', '..XO..', '......'], ['.OOO..', '..OXX.', '..XX..', '..X...'], ['.OOO..', '..OOX.', '..XO..', '..XO..'], ['.OOO..', '..OOX.', '..XO..', '..XXX.'], ['.OOO.O', '..OOO.', '..XO..', '..XXX.'], ['.OOO.O', '..OOO.', '..XXX.', '..XXX.'], ['.OOO.O', '..OOO.', '..XXO.', '..XXXO'], ['.OOOXO', '..OXX.', '..XXX.', '..XXXO'], ['.OOOXO', '..OXX.', '..XXX.', '.OOOOO'], ['XXXXXO', '..OXX.', '..XXX.', '.OOOOO'], ['XXXXXO', '.OOXX.', '..OXX.', '.OOOOO'], ['XXXXXO', 'XXXXX.', '..OXX.', '.OOOOO'], ['XXXXXO', 'XXXXX.', '..OOOO', '.OOOOO']], 0.0, True, None),
    _case('edge_run_without_anchor', 'N', [21, 22, 16],
          [['......', '..OX..', '..XX..', '...X..'], ['......', '..OX..', '..XO..', '...XO.'], ['......', '..OX..', '..XXX.', '...XO.']]),
    _case('end_full_board', 'N', [16, 22, 7, 1, 21, 13, 12, 10, 11, 20, 6, 0, 19, 2, 3, 23, 17, 18, 4, 5],
          [['......', '..OX..', '..XXX.', '......'], ['......', '..OX..', '..XOX.', '....O.'], ['......', '.XXX..', '..XOX.', '....O.'], ['.O....', '.XOX..', '..XOX.', '....O.'], ['.O....', '.XOX..', '..XXX.', '...XO.'], ['.O....', '.OOX..', '.OXXX.', '...XO.'], ['.O....', '.OOX..', 'XXXXX.', '...XO.'], ['.O....', '.OOOO.', 'XXXXO.', '...XO.'], ['.O....', '.OOOOX', 'XXXXX.', '...XO.'], ['.O....', '.OOOOX', 'XXOOX.', '..OOO.'], ['.O....', 'XXXXXX', 'XXOOX.', '..OOO.'], ['OO....', 'XOXXXX', 'XXOOX.', '..OOO.'], ['OO....', 'XOXXXX', 'XXXOX.', '.XOOO.'], ['OOO...', 'XOOXXX', 'XXOOX.', '.XOOO.'], ['OOOX..', 'XOXXXX', 'XXOOX.', '.XOOO.'], ['OOOX..', 'XOXOXX', 'XXOOO.', '.XOOOO'], ['OOOX..', 'XOXOXX', 'XXXXXX', '.XOOOO'], ['OOOX..', 'OOXOXX', 'OXXXXX', 'OOOOOO'], ['OOOXX.', 'OOXXXX', 'OXXXXX', 'OOOOOO'], ['OOOOOO', 'OOXXOO', 'OXXOXO', 'OOOOOO']], 1.0, True, 2),
    _case('end_with_empty_cells', 'N', [21, 10, 5, 19, 3, 4, 7, 2, 1],
          [['......', '..OX..', '..XX..', '...X..'], ['......', '..OOO.', '..XX..', '...X..'], ['.....X', '..OOX.', '..XX..', '...X..'], ['.....X', '..OOX.', '..OX..', '.O.X..'], ['...X.X', '..OXX.', '..OX..', '.O.X..'], ['...XOX', '..OOX.', '..OX..', '.O.X..'], ['...XOX', '.XXXX.', '..XX..', '.O.X..'], ['..OOOX', '.XXXX.', '..XX..', '.O.X..'], ['.XXXXX', '.XXXX.', '..XX..', '.O.X..']], 1.0, True, 1),
    _case('final_placement_loses', 'N', [2, 1, 0, 3, 4, 20, 21, 22, 19, 7, 6, 18],
          [['..X...', '..XX..', '..XO..', '......'], ['.OX...', '..OX..', '..XO..', '......'], ['XXX...', '..OX..', '..XO..', '......'], ['XXXO..', '..OO..', '..XO..', '......'], ['XXXXX.', '..OX..', '..XO..', '......'], ['XXXXX.', '..OX..', '..OO..', '..O...'], ['XXXXX.', '..OX..', '..OX..', '..OX..'], ['XXXXX.', '..OX..', '..OO..', '..OOO.'], ['XXXXX.', '..OX..', '..XO..', '.XOOO.'], ['XXXXX.', '.OOX..', '..OO..', '.XOOO.'], ['XXXXX.', 'XXXX..', '..OO..', '.XOOO.'], ['XXXXX.', 'XXXX..', '..OO..', 'OOOOO.']], -1.0, True, 1),
    _case('flip_east', 'N', [7],
          [['......', '.XXX..', '..XO..', '......']]),
    _case('flip_north', 'N', [21],
          [['......', '..OX..', '..XX..', '...X..']]),
    _case('flip_north_east', 'N', [7, 13, 18],
          [['......', '.XXX..', '..XO..', '......'], ['......', '.XXX..', '.OOO..', '......'], ['......', '.XXX..', '.XOO..', 'X.....']]),
    _case('flip_north_west', 'N', [21, 22],
          [['......', '..OX..', '..XX..', '...X..'], ['......', '..OX..', '..XO..', '...XO.']]),
    _case('flip_south', 'N', [2],
          [['..X...', '..XX..', '..XO..', '......']]),
    _case('flip_south_east', 'N', [7, 1],
          [['......', '.XXX..', '..XO..', '......'], ['.O....', '.XOX..', '..XO..', '......']]),
    _case('flip_south_west', 'N', [21, 10, 4],
          [['......', '..OX..', '..XX..', '...X..'], ['......', '..OOO.', '..XX..', '...X..'], ['....X.', '..OXO.', '..XX..', '...X..']]),
    _case('flip_three_directions', 'N', [16, 22, 21, 20, 19, 10],
          [['......', '..OX..', '..XXX.', '......'], ['......', '..OX..', '..XOX.', '....O.'], ['......', '..OX..', '..XXX.', '...XO.'], ['......', '..OX..', '..OXX.', '..OOO.'], ['......', '..OX..', '..XXX.', '.XOOO.'], ['......', '..OOO.', '..XOO.', '.XOOO.']]),
    _case('flip_west', 'N', [16],
          [['......', '..OX..', '..XXX.', '......']]),
    _case('flipped_twice', 'N', [21, 22],
          [['......', '..OX..', '..XX..', '...X..'], ['......', '..OX..', '..XO..', '...XO.']]),
    _case('forced_pass', 'N', [21, 20, 7, 22, 24],
          [['......', '..OX..', '..XX..', '...X..'], ['......', '..OX..', '..OX..', '..OX..'], ['......', '.XXX..', '..XX..', '..OX..'], ['......', '.XXX..', '..XX..', '..OOO.'], ['......', '.XXX..', '..XX..', '..OOO.']]),
    _case('run_broken_by_empty', 'N', [2, 1, 0, 20, 21],
          [['..X...', '..XX..', '..XO..', '......'], ['.OX...', '..OX..', '..XO..', '......'], ['XXX...', '..OX..', '..XO..', '......'], ['XXX...', '..OX..', '..OO..', '..O...'], ['XXX...', '..OX..', '..OX..', '..OX..']]),
    _case('two_passes_same_side', 'N', [2, 3, 16, 13, 1, 17, 4, 24, 22, 24],
          [['..X...', '..XX..', '..XO..', '......'], ['..XO..', '..XO..', '..XO..', '......'], ['..XO..', '..XX..', '..XXX.', '......'], ['..XO..', '..OX..', '.OXXX.', '......'], ['.XXO..', '..XX..', '.OXXX.', '......'], ['.XXO..', '..XX..', '.OOOOO', '......'], ['.XXXX.', '..XX..', '.OOOOO', '......'], ['.XXXX.', '..XX..', '.OOOOO', '......'], ['.XXXX.', '..XX..', '.OOXOO', '....X.'], ['.XXXX.', '..XX..', '.OOXOO', '....X.']]),
    _case('wipe_out', 'N', [16, 22, 2, 17, 21, 13, 20, 19, 23, 7, 12, 11, 18, 24, 5, 24, 10],
          [['......', '..OX..', '..XXX.', '......'], ['......', '..OX..', '..XOX.', '....O.'], ['..X...', '..XX..', '..XOX.', '....O.'], ['..X...', '..XX..', '..XOOO', '....O.'], ['..X...', '..XX..', '..XXOO', '...XO.'], ['..X...', '..XX..', '.OOOOO', '...XO.'], ['..X...', '..XX..', '.OXOOO', '..XXO.'], ['..X...', '..XX..', '.OXOOO', '.OOOO.'], ['..X...', '..XX..', '.OXOXO', '.OOOOX'], ['..X...', '.OXX..', '.OOOXO', '.OOOOX'], ['..X...', '.XXX..', 'XXXXXO', '.OOOOX'], ['..X...', '.XXX.O', 'XXXXOO', '.OOOOX'], ['..X...', '.XXX.O', 'XXXXOO', 'XXXXXX'], ['..X...', '.XXX.O', 'XXXXOO', 'XXXXXX'], ['..X..X', '.XXX.X', 'XXXXOX', 'XXXXXX'], ['..X..X', '.XXX.X', 'XXXXOX', 'XXXXXX'], ['..X..X', '.XXXXX', 'XXXXXX', 'XXXXXX']], 1.0, True, 1),
    _case('wrap_east', 'N', [16, 22, 2, 17],
          [['......', '..OX..', '..XXX.', '......'], ['......', '..OX..', '..XOX.', '....O.'], ['..X...', '..XX..', '..XOX.', '....O.'], ['..X...', '..XX..', '..XOOO', '....O.']]),
    _case('wrap_north_east', 'N', [16, 10, 4, 11],
          [['......', '..OX..', '..XXX.', '......'], ['......', '..OOO.', '..XXX.', '......'], ['....X.', '..OXX.', '..XXX.', '......'], ['....X.', '..OOOO', '..XXX.', '......']]),
    _case('wrap_north_west', 'N', [7, 13, 19, 12],
          [['......', '.XXX..', '..XO..', '......'], ['......', '.XXX..', '.OOO..', '......'], ['......', '.XXX..', '.XXO..', '.X....'], ['......', '.XXX..', 'OOOO..', '.X....']]),
    _case('wrap_south_east', 'N', [16, 10, 4, 11],
          [['......', '..OX..', '..XXX.', '......'], ['......', '..OOO.', '..XXX.', '......'], ['....X.', '..OXX.', '..XXX.', '......'], ['....X.', '..OOOO', '..XXX.', '......']]),
    _case('wrap_south_west', 'N', [7, 13, 19, 12],
          [['......', '.XXX..', '..XO..', '......'], ['......', '.XXX..', '.OOO..', '......'], ['......', '.XXX..', '.XXO..', '.X....'], ['......', '.XXX..', 'OOOO..', '.X....']]),
    _case('wrap_west', 'N', [7, 1, 21, 6],
          [['......', '.XXX..', '..XO..', '......'], ['.O....', '.XOX..', '..XO..', '......'], ['.O....', '.XOX..', '..XX..', '...X..'], ['.O....', 'OOOX..', '..XX..', '...X..']]),
    _case('resign_black', 'N', [25], [['......', '..OX..', '..XO..', '......']], -1.0, True, 2),
    _case('resign_white', 'N', [2, 25], [['..X...', '..XX..', '..XO..', '......'], ['..X...', '..XX..', '..XO..', '......']], -1.0, True, 1),
    # ---- M: 6 x 6 ----
    _case('end_full_board', 'M', [8, 19, 26, 31, 22, 9, 10, 4, 7, 6, 2, 11, 24, 25, 0, 1, 32, 29, 5, 18, 17, 16, 28, 13, 27, 33, 23, 30, 12, 3, 34, 35],
          [['......', '..X...', '..XX..', '..XO..', '......', '......'], ['......', '..X...', '..XX..', '.OOO..', '......', '......'], ['......', '..X...', '..XX..', '.OXO..', '..X...', '......'], ['......', '..X...', '..XX..', '.OXO..', '..O...', '.O....'], ['......', '..X...', '..XX..', '.OXXX.', '..O...', '.O....'], ['......', '..XO..', '..OX..', '.OXXX.', '..O...', '.O....'], ['......', '..XXX.', '..OX..', '.OXXX.', '..O...', '.O....'], ['....O.', '..XOX.', '..OX..', '.OXXX.', '..O...', '.O....'], ['....O.', '.XXOX.', '..XX..', '.OXXX.', '..O...', '.O....'], ['....O.', 'OOOOX.', '..XX..', '.OXXX.', '..O...', '.O....'], ['..X.O.', 'OOXOX.', '..XX..', '.OXXX.', '..O...', '.O....'], ['..X.O.', 'OOXOOO', '..XX..', '.OXXX.', '..O...', '.O....'], ['..X.O.', 'OOXOOO', '..XX..', '.XXXX.', 'X.O...', '.O....'], ['..X.O.', 'OOXOOO', '..XO..', '.XOXX.', 'XOO...', '.O....'], ['X.X.O.', 'OXXOOO', '..XO..', '.XOXX.', 'XOO...', '.O....'], ['XOX.O.', 'OXOOOO', '..XO..', '.XOXX.', 'XOO...', '.O....'], ['XOX.O.', 'OXOOOO', '..XO..', '.XXXX.', 'XOX...', '.OX...'], ['XOX.O.', 'OXOOOO', '..XO..', '.XXXO.', 'XOX..O', '.OX...'], ['XOX.OX', 'OXOOXO', '..XX..', '.XXXO.', 'XOX..O', '.OX...'], ['XOX.OX', 'OXOOXO', '..XX..', 'OOOOO.', 'XOX..O', '.OX...'], ['XOX.OX', 'OXOOXX', '..XX.X', 'OOOOO.', 'XOX..O', '.OX...'], ['XOX.OX', 'OXOOOX', '..XXOX', 'OOOOO.', 'XOX..O', '.OX...'], ['XOX.OX', 'OXOOOX', '..XXOX', 'OOOXO.', 'XOX.XO', '.OX...'], ['XOX.OX', 'OOOOOX', '.OOOOX', 'OOOXO.', 'XOX.XO', '.OX...'], ['XOX.OX', 'OOOOOX', '.OOOOX', 'OOOXX.', 'XOXXXO', '.OX...'], ['XOX.OX', 'OOOOOX', '.OOOOX', 'OOOOX.', 'XOOOXO', '.OOO..'], ['XOX.OX', 'OOOXOX', '.OOOXX', 'OOOOXX', 'XOOOXO', '.OOO..'], ['XOX.OX', 'OOOXOX', '.OOOXX', 'OOOOXX', 'OOOOXO', 'OOOO..'], ['XOX.OX', 'XXOXOX', 'XXXXXX', 'OOOOXX', 'OOOOXO', 'OOOO..'], ['XOOOOX', 'XXOOOX', 'XXXOXX', 'OOOOXX', 'OOOOXO', 'OOOO..'], ['XOOOOX', 'XXOOOX', 'XXXOXX', 'OOXOXX', 'OOOXXO', 'OOOOX.'], ['XOOOOX', 'XXOOOX', 'XXXOXX', 'OOXOXX', 'OOOXOO', 'OOOOOO']], 1.0, True, 2),
    _case('end_with_empty_cells', 'M', [22, 26, 25, 16, 10, 17, 32, 29, 8, 31, 23, 30, 19, 12, 18, 24, 33, 4, 9, 1, 7, 2, 35, 28, 0, 27, 11, 5, 3, 34, 36, 13],
          [['......', '......', '..OX..', '..XXX.', '......', '......'], ['......', '......', '..OX..', '..OXX.', '..O...', '......'], ['......', '......', '..OX..', '..XXX.', '.XO...', '......'], ['......', '......', '..OOO.', '..XOX.', '.XO...', '......'], ['......', '....X.', '..OXX.', '..XOX.', '.XO...', '......'], ['......', '....X.', '..OOOO', '..XOX.', '.XO...', '......'], ['......', '....X.', '..OOOO', '..XOX.', '.XX...', '..X...'], ['......', '....X.', '..OOOO', '..XOO.', '.XX..O', '..X...'], ['......', '..X.X.', '..XOOO', '..XOO.', '.XX..O', '..X...'], ['......', '..X.X.', '..XOOO', '..XOO.', '.XO..O', '.OX...'], ['......', '..X.X.', '..XOOO', '..XXXX', '.XO..O', '.OX...'], ['......', '..X.X.', '..XOOO', '..OXXX', '.OO..O', 'OOX...'], ['......', '..X.X.', '..XOOO', '.XXXXX', '.OO..O', 'OOX...'], ['......', '..X.X.', 'O.XOOO', '.OXXXX', '.OO..O', 'OOX...'], ['......', '..X.X.', 'O.XOOO', 'XXXXXX', '.XO..O', 'OOX...'], ['......', '..X.X.', 'O.XOOO', 'OXXXXX', 'OOO..O', 'OOX...'], ['......', '..X.X.', 'O.XOOO', 'OXXXXX', 'OOX..O', 'OOXX..'], ['....O.', '..X.O.', 'O.XOOO', 'OXXXXX', 'OOX..O', 'OOXX..'], ['....O.', '..XXO.', 'O.XXXO', 'OXXXXX', 'OOX..O', 'OOXX..'], ['.O..O.', '..OXO.', 'O.XOXO', 'OXXXOX', 'OOX..O', 'OOXX..'], ['.O..O.', '.XXXO.', 'O.XOXO', 'OXXXOX', 'OOX..O', 'OOXX..'], ['.OO.O.', '.OXXO.', 'O.XOXO', 'OXXXOX', 'OOX..O', 'OOXX..'], ['.OO.O.', '.OXXO.', 'O.XOXO', 'OXXXOX', 'OOX..X', 'OOXX.X'], ['.OO.O.', '.OXXO.', 'O.OOXO', 'OXXOOX', 'OOX.OX', 'OOXX.X'], ['XOO.O.', '.XXXO.', 'O.XOXO', 'OXXXOX', 'OOX.XX', 'OOXX.X'], ['XOO.O.', '.XXXO.', 'O.XOXO', 'OXXOOX', 'OOOOXX', 'OOXX.X'], ['XOO.O.', '.XXXXX', 'O.XOXX', 'OXXOOX', 'OOOOXX', 'OOXX.X'], ['XOO.OO', '.XXXOX', 'O.XOXX', 'OXXOOX', 'OOOOXX', 'OOXX.X'], ['XXXXOO', '.XXXXX', 'O.XOXX', 'OXXOOX', 'OOOOXX', 'OOXX.X'], ['XXXXOO', '.XXXXX', 'O.XOXX', 'OXXOOX', 'OOOOOX', 'OOOOOX'], ['XXXXOO', '.XXXXX', 'O.XOXX', 'OXXOOX', 'OOOOOX', 'OOOOOX'], ['XXXXOO', '.XXXXX', 'OOOOXX', 'OOOOOX', 'OOOOOX', 'OOOOOX']], 1.0, True, 2),
    _case('flip_three_directions', 'M', [27, 28, 22, 26, 32, 16],
          [['......', '......', '..OX..', '..XX..', '...X..', '......'], ['......', '......', '..OX..', '..XO..', '...XO.', '......'], ['......', '......', '..OX..', '..XXX.', '...XO.', '......'], ['......', '......', '..OX..', '..OXX.', '..OOO.', '......'], ['......', '......', '..OX..', '..OXX.', '..OXO.', '..X...'], ['......', '......', '..OOO.', '..OOO.', '..OXO.', '..X...']]),
    _case('forced_pass', 'M', [8, 9, 10, 3, 22, 17, 11, 5, 36],
          [['......', '..X...', '..XX..', '..XO..', '......', '......'], ['......', '..XO..', '..XO..', '..XO..', '......', '......'], ['......', '..XXX.', '..XX..', '..XO..', '......', '......'], ['...O..', '..XOX.', '..XO..', '..XO..', '......', '......'], ['...O..', '..XOX.', '..XX..', '..XXX.', '......', '......'], ['...O..', '..XOO.', '..XX.O', '..XXX.', '......', '......'], ['...O..', '..XXXX', '..XX.O', '..XXX.', '......', '......'], ['...O.O', '..XXXO', '..XX.O', '..XXX.', '......', '......'], ['...O.O', '..XXXO', '..XX.O', '..XXX.', '......', '......']]),
    _case('two_passes_same_side', 'M', [8, 9, 16, 11, 27, 13, 18, 7, 3, 4, 10, 19, 0, 1, 2, 26, 12, 6, 5, 34, 25, 24, 31, 22, 30, 36, 32, 36],
          [['......', '..X...', '..XX..', '..XO..', '......', '......'], ['......', '..XO..', '..XO..', '..XO..', '......', '......'], ['......', '..XO..', '..XXX.', '..XO..', '......', '......'], ['......', '..XO.O', '..XXO.', '..XO..', '......', '......'], ['......', '..XO.O', '..XXO.', '..XX..', '...X..', '......'], ['......', '..XO.O', '.OOOO.', '..XX..', '...X..', '......'], ['......', '..XO.O', '.XOOO.', 'X.XX..', '...X..', '......'], ['......', '.OOO.O', '.XOOO.', 'X.XX..', '...X..', '......'], ['...X..', '.OXX.O', '.XOXO.', 'X.XX..', '...X..', '......'], ['...XO.', '.OXO.O', '.XOXO.', 'X.XX..', '...X..', '......'], ['...XO.', '.OXXXO', '.XOXO.', 'X.XX..', '...X..', '......'], ['...XO.', '.OXXXO', '.OOXO.', 'XOXX..', '...X..', '......'], ['X..XO.', '.XXXXO', '.OXXO.', 'XOXX..', '...X..', '......'], ['XO.XO.', '.OXXXO', '.OXXO.', 'XOXX..', '...X..', '......'], ['XXXXO.', '.OXXXO', '.OXXO.', 'XOXX..', '...X..', '......'], ['XXXXO.', '.OXXXO', '.OXXO.', 'XOXO..', '..OX..', '......'], ['XXXXO.', '.XXXXO', 'XXXXO.', 'XOXO..', '..OX..', '......'], ['XXXXO.', 'OOOOOO', 'XXXXO.', 'XOXO..', '..OX..', '......'], ['XXXXXX', 'OOOOXO', 'XXXXO.', 'XOXO..', '..OX..', '......'], ['XXXXXX', 'OOOOXO', 'XOXXO.', 'XOOO..', '..OO..', '....O.'], ['XXXXXX', 'OXOOXO', 'XXXXO.', 'XXXO..', '.XOO..', '....O.'], ['XXXXXX', 'OXOOXO', 'OXOXO.', 'OOXO..', 'OOOO..', '....O.'], ['XXXXXX', 'OXOOXO', 'OXOXO.', 'OXXO..', 'OXOO..', '.X..O.'], ['XXXXXX', 'OXOOXO', 'OXOOO.', 'OXXOO.', 'OXOO..', '.X..O.'], ['XXXXXX', 'XXOOXO', 'XXOOO.', 'XXXOO.', 'XXOO..', 'XX..O.'], ['XXXXXX', 'XXOOXO', 'XXOOO.', 'XXXOO.', 'XXOO..', 'XX..O.'], ['XXXXXX', 'XXOOXO', 'XXOOO.', 'XXXOO.', 'XXXO..', 'XXX.O.'], ['XXXXXX', 'XXOOXO', 'XXOOO.', 'XXXOO.', 'XXXO..', 'XXX.O.']]),
    _case('resign_black', 'M', [37], [['......', '......', '..OX..', '..XO..', '......', '......']], -1.0, True, 2),
    _case('resign_white', 'M', [8, 37], [['......', '..X...', '..XX..', '..XO..', '......', '......'], ['......', '..X...', '..XX..', '..XO..', '......', '......']], -1.0, True, 1),
    # ---- F: 8 x 8 ----
    _case('end_full_board', 'F', [44, 45, 46, 54, 37, 43, 18, 19, 53, 29, 55, 62, 10, 9, 42, 11, 26, 50, 0, 63, 61, 17, 25, 32, 58, 16, 60, 41, 33, 47, 34, 57, 52, 2, 4, 51, 1, 30, 49, 3, 12, 24, 31, 56, 40, 13, 22, 23, 8, 20, 38, 14, 6, 59, 5, 21, 39, 7, 15, 48],
          [['........', '........', '........', '...OX...', '...XX...', '....X...', '........', '........'], ['........', '........', '........', '...OX...', '...XO...', '....XO..', '........', '........'], ['........', '........', '........', '...OX...', '...XO...', '....XXX.', '........', '........'], ['........', '........', '........', '...OX...', '...XO...', '....XOX.', '......O.', '........'], ['........', '........', '........', '...OX...', '...XXX..', '....XOX.', '......O.', '........'], ['........', '........', '........', '...OX...', '...OXX..', '...OOOX.', '......O.', '........'], ['........', '........', '..X.....', '...XX...', '...OXX..', '...OOOX.', '......O.', '........'], ['........', '........', '..XO....', '...OX...', '...OXX..', '...OOOX.', '......O.', '........'], ['........', '........', '..XO....', '...OX...', '...OXX..', '...OOXX.', '.....XO.', '........'], ['........', '........', '..XO....', '...OOO..', '...OOX..', '...OOXX.', '.....XO.', '........'], ['........', '........', '..XO....', '...OOO..', '...OOX..', '...OOXX.', '.....XXX', '........'], ['........', '........', '..XO....', '...OOO..', '...OOX..', '...OOXX.', '.....OXX', '......O.'], ['........', '..X.....', '..XX....', '...OXO..', '...OOX..', '...OOXX.', '.....OXX', '......O.'], ['........', '.OX.....', '..OX....', '...OXO..', '...OOX..', '...OOXX.', '.....OXX', '......O.'], ['........', '.OX.....', '..OX....', '...OXO..', '...XOX..', '..XXXXX.', '.....OXX', '......O.'], ['........', '.OOO....', '..OO....', '...OXO..', '...XOX..', '..XXXXX.', '.....OXX', '......O.'], ['........', '.OOO....', '..OO....', '..XXXO..', '...XOX..', '..XXXXX.', '.....OXX', '......O.'], ['........', '.OOO....', '..OO....', '..XXXO..', '...XOX..', '..XOXXX.', '..O..OXX', '......O.'], ['X.......', '.XOO....', '..XO....', '..XXXO..', '...XOX..', '..XOXXX.', '..O..OXX', '......O.'], ['X.......', '.XOO....', '..XO....', '..XXXO..', '...XOX..', '..XOXOX.', '..O..OOX', '......OO'], ['X.......', '.XOO....', '..XO....', '..XXXO..', '...XOX..', '..XOXXX.', '..O..XOX', '.....XOO'], ['X.......', '.XOO....', '.OOO....', '..OXXO..', '...OOX..', '..XOOXX.', '..O..OOX', '.....XOO'], ['X.......', '.XOO....', '.XOO....', '.XXXXO..', '...OOX..', '..XOOXX.', '..O..OOX', '.....XOO'], ['X.......', '.XOO....', '.XOO....', '.OXXXO..', 'O..OOX..', '..XOOXX.', '..O..OOX', '.....XOO'], ['X.......', '.XOO....', '.XOO....', '.OXXXO..', 'O..OOX..', '..XOOXX.', '..X..OOX', '..X..XOO'], ['X.......', '.XOO....', 'OOOO....', '.OXXXO..', 'O..OOX..', '..XOOXX.', '..X..OOX', '..X..XOO'], ['X.......', '.XOO....', 'OOOO....', '.OXXXO..', 'O..OOX..', '..XOOXX.', '..X..XOX', '..X.XXOO'], ['X.......', '.XOO....', 'OOOO....', '.OXXXO..', 'O..OOX..', '.OOOOXX.', '..X..XOX', '..X.XXOO'], ['X.......', '.XOO....', 'OXOO....', '.XXXXO..', 'OX.OOX..', '.OOOOXX.', '..X..XOX', '..X.XXOO'], ['X.......', '.XOO....', 'OXOO....', '.XXXXO..', 'OX.OOX..', '.OOOOOOO', '..X..XOO', '..X.XXOO'], ['X.......', '.XOO....', 'OXOO....', '.XXXXO..', 'OXXXXX..', '.OXOOOOO', '..X..XOO', '..X.XXOO'], ['X.......', '.XOO....', 'OXOO....', '.XXXXO..', 'OXXXXX..', '.OXOOOOO', '..O..XOO', '.OX.XXOO'], ['X.......', '.XOO....', 'OXOO....', '.XXXXO..', 'OXXXXX..', '.OXXXOOO', '..O.XXOO', '.OX.XXOO'], ['X.O.....', '.OOO....', 'OXOO....', '.XXXXO..', 'OXXXXX..', '.OXXXOOO', '..O.XXOO', '.OX.XXOO'], ['X.O.X...', '.OOX....', 'OXXO....', '.XXXXO..', 'OXXXXX..', '.OXXXOOO', '..O.XXOO', '.OX.XXOO'], ['X.O.X...', '.OOX....', 'OXXO....', '.XXOXO..', 'OXXOXX..', '.OXOXOOO', '..OOOOOO', '.OX.XXOO'], ['XXO.X...', '.XXX....', 'OXXX....', '.XXOXO..', 'OXXOXX..', '.OXOXOOO', '..OOOOOO', '.OX.XXOO'], ['XXO.X...', '.XXX....', 'OXXX....', '.XXOXOO.', 'OXXOXO..', '.OXOOOOO', '..OOOOOO', '.OX.XXOO'], ['XXO.X...', '.XXX....', 'OXXX....', '.XXOXOO.', 'OXXOXO..', '.XXOOOOO', '.XOOOOOO', '.OX.XXOO'], ['XXOOX...', '.XXO....', 'OXXO....', '.XXOXOO.', 'OXXOXO..', '.XXOOOOO', '.XOOOOOO', '.OX.XXOO'], ['XXOOX...', '.XXXX...', 'OXXX....', '.XXOXOO.', 'OXXOXO..', '.XXOOOOO', '.XOOOOOO', '.OX.XXOO'], ['XXOOX...', '.XOXX...', 'OOXX....', 'OOOOXOO.', 'OOXOXO..', '.XOOOOOO', '.XOOOOOO', '.OX.XXOO'], ['XXOOX...', '.XOXX...', 'OOXX....', 'OOOOXXXX', 'OOXOXO..', '.XOOOOOO', '.XOOOOOO', '.OX.XXOO'], ['XXOOX...', '.XOXX...', 'OOXX....', 'OOOOXXXX', 'OOXOXO..', '.XOOOOOO', '.OOOOOOO', 'OOX.XXOO'], ['XXOOX...', '.XOXX...', 'OOXX....', 'OOXOXXXX', 'OXXOXO..', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', '.XOOOO..', 'OOXX....', 'OOXOXXXX', 'OXXOXO..', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', '.XOOOX..', 'OOXX..X.', 'OOXOXXXX', 'OXXOXO..', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', '.XOOOX..', 'OOXX..XO', 'OOXOXXOX', 'OXXOXO..', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', 'XXOOOX..', 'XXXX..XO', 'XOXOXXOX', 'XXXOXO..', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', 'XXOOOX..', 'XXXXO.XO', 'XOXOOXOX', 'XXXOOO..', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', 'XXOOOX..', 'XXXXO.XO', 'XOXOOXXX', 'XXXXXXX.', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX...', 'XXOOOOO.', 'XXXXO.OO', 'XOXOOXOX', 'XXXXXXO.', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX.X.', 'XXOOOXO.', 'XXXXX.OO', 'XOXXOXOX', 'XXXXXXO.', 'XXOOOOOO', '.XOOOOOO', 'OOX.XXOO'], ['XXOOX.X.', 'XXOOOXO.', 'XXXXX.OO', 'XOXXOXOX', 'XXXXXXO.', 'XXOOOOOO', '.XOOOOOO', 'OOOOOOOO'], ['XXOOXXX.', 'XXOOXXO.', 'XXXXX.OO', 'XOXXOXOX', 'XXXXXXO.', 'XXOOOOOO', '.XOOOOOO', 'OOOOOOOO'], ['XXOOXXX.', 'XXOOOXO.', 'XXXXXOOO', 'XOXXOOOX', 'XXXXXOO.', 'XXOOOOOO', '.XOOOOOO', 'OOOOOOOO'], ['XXOOXXX.', 'XXOOOXO.', 'XXXXXOOO', 'XOXXOOOX', 'XXXXXXXX', 'XXOOOOOO', '.XOOOOOO', 'OOOOOOOO'], ['XXOOOOOO', 'XXOOOXO.', 'XXXXXOOO', 'XOXXOOOX', 'XXXXXXXX', 'XXOOOOOO', '.XOOOOOO', 'OOOOOOOO'], ['XXOOOOOO', 'XXOOOXXX', 'XXXXXOXX', 'XOXXOXOX', 'XXXXXXXX', 'XXOOOOOO', '.XOOOOOO', 'OOOOOOOO'], ['XXOOOOOO', 'XXOOOOXX', 'XXXXOOXX', 'XOXOOXOX', 'XXOXXXXX', 'XOOOOOOO', 'OOOOOOOO', 'OOOOOOOO']], 1.0, True, 2),
    _case('forced_pass', 'F', [19, 34, 43, 52, 33, 25, 45, 38, 41, 29, 37, 32, 44, 51, 54, 53, 59, 49, 48, 42, 57, 26, 46, 39, 16, 10, 17, 50, 18, 62, 63, 20, 61, 24, 31, 60, 11, 12, 9, 58, 40, 47, 30, 8, 13, 14, 2, 22, 15, 56, 55, 21, 64],
          [['........', '........', '...X....', '...XX...', '...XO...', '........', '........', '........'], ['........', '........', '...X....', '...XX...', '..OOO...', '........', '........', '........'], ['........', '........', '...X....', '...XX...', '..OXO...', '...X....', '........', '........'], ['........', '........', '...X....', '...XX...', '..OXO...', '...O....', '....O...', '........'], ['........', '........', '...X....', '...XX...', '.XXXO...', '...O....', '....O...', '........'], ['........', '........', '...X....', '.O.XX...', '.XOXO...', '...O....', '....O...', '........'], ['........', '........', '...X....', '.O.XX...', '.XOXX...', '...O.X..', '....O...', '........'], ['........', '........', '...X....', '.O.XX...', '.XOXX.O.', '...O.O..', '....O...', '........'], ['........', '........', '...X....', '.O.XX...', '.XXXX.O.', '.X.O.O..', '....O...', '........'], ['........', '........', '...X....', '.O.XXO..', '.XXXO.O.', '.X.O.O..', '....O...', '........'], ['........', '........', '...X....', '.O.XXO..', '.XXXXXO.', '.X.O.O..', '....O...', '........'], ['........', '........', '...X....', '.O.XXO..', 'OOOOOOO.', '.X.O.O..', '....O...', '........'], ['........', '........', '...X....', '.O.XXO..', 'OOOOXOO.', '.X.OXO..', '....O...', '........'], ['........', '........', '...X....', '.O.XXO..', 'OOOOXOO.', '.X.OOO..', '...OO...', '........'], ['........', '........', '...X....', '.O.XXO..', 'OOOOXOO.', '.X.OOX..', '...OO.X.', '........'], ['........', '........', '...X....', '.O.XXO..', 'OOOOXOO.', '.X.OOO..', '...OOOX.', '........'], ['........', '........', '...X....', '.O.XXO..', 'OOOXXOO.', '.X.XOO..', '...XOOX.', '...X....'], ['........', '........', '...X....', '.O.XXO..', 'OOOXXOO.', '.O.XOO..', '.O.XOOX.', '...X....'], ['........', '........', '...X....', '.O.XXO..', 'OOXXXOO.', '.X.XOO..', 'XO.XOOX.', '...X....'], ['........', '........', '...X....', '.O.XXO..', 'OOXXXOO.', '.XOOOO..', 'XO.XOOX.', '...X....'], ['........', '........', '...X....', '.O.XXO..', 'OOXXXOO.', '.XOOOO..', 'XX.XOOX.', '.X.X....'], ['........', '........', '...X....', '.OOOOO..', 'OOOOXOO.', '.XOOOO..', 'XX.XOOX.', '.X.X....'], ['........', '........', '...X....', '.OOOXO..', 'OOOOXXO.', '.XXXXXX.', 'XX.XOOX.', '.X.X....'], ['........', '........', '...X....', '.OOOXO..', 'OOOOXXOO', '.XXXXXO.', 'XX.XOOX.', '.X.X....'], ['........', '........', 'X..X....', '.XOOXO..', 'OOXOXXOO', '.XXXXXO.', 'XX.XOOX.', '.X.X....'], ['........', '..O.....', 'X..O....', '.XOOOO..', 'OOXOXOOO', '.XXXXXO.', 'XX.XOOX.', '.X.X....'], ['........', '..O.....', 'XX.O....', '.XXOOO..', 'OOXXXOOO', '.XXXXXO.', 'XX.XOOX.', '.X.X....'], ['........', '..O.....', 'XX.O....', '.XXOOO..', 'OOXXOOOO', '.OXOXXO.', 'XXOOOOX.', '.X.X....'], ['........', '..O.....', 'XXXO....', '.XXXOO..', 'OOXXXOOO', '.OXOXXO.', 'XXOOOOX.', '.X.X....'], ['........', '..O.....', 'XXXO....', '.XXXOO..', 'OOXXXOOO', '.OXOXXO.', 'XXOOOOO.', '.X.X..O.'], ['........', '..O.....', 'XXXO....', '.XXXOO..', 'OOXXXOOO', '.OXOXXO.', 'XXOOOOX.', '.X.X..OX'], ['........', '..O.....', 'XXXOO...', '.XXOOO..', 'OOOXXOOO', '.OXOXXO.', 'XXOOOOX.', '.X.X..OX'], ['........', '..O.....', 'XXXOO...', '.XXOOO..', 'OOXXXOOO', '.OXXXXO.', 'XXOOXXX.', '.X.X.XXX'], ['........', '..O.....', 'XOXOO...', 'OOOOOO..', 'OOXXXOOO', '.OXXXXO.', 'XXOOXXX.', '.X.X.XXX'], ['........', '..O.....', 'XOXOO...', 'OOOOOO.X', 'OOXXXOXO', '.OXXXXO.', 'XXOOXXX.', '.X.X.XXX'], ['........', '..O.....', 'XOXOO...', 'OOOOOO.X', 'OOXXOOXO', '.OXXOXO.', 'XXOOOOX.', '.X.XOXXX'], ['........', '..OX....', 'XOXXX...', 'OOOXOX.X', 'OOXXOOXO', '.OXXOXO.', 'XXOOOOX.', '.X.XOXXX'], ['........', '..OOO...', 'XOXOO...', 'OOOXOX.X', 'OOXXOOXO', '.OXXOXO.', 'XXOOOOX.', '.X.XOXXX'], ['........', '.XOOO...', 'XXXOO...', 'OXOXOX.X', 'OXXXOOXO', '.XXXOXO.', 'XXOOOOX.', '.X.XOXXX'], ['........', '.XOOO...', 'XXXOO...', 'OXOXOX.X', 'OXXXOOXO', '.XXXOXO.', 'XXOOOOX.', '.XOOOXXX'], ['........', '.XOOO...', 'XXXOO...', 'XXOXOX.X', 'XXXXOOXO', 'XXXXOXO.', 'XXOOOOX.', '.XOOOXXX'], ['........', '.XOOO...', 'XXXOO...', 'XXOXOO.X', 'XXXXOOOO', 'XXXXOXOO', 'XXOOOOX.', '.XOOOXXX'], ['........', '.XOOO...', 'XXXOO...', 'XXOXXXXX', 'XXXXOOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['........', 'OOOOO...', 'XOXOO...', 'XXOXXXXX', 'XXXXOOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['........', 'OOOOOX..', 'XOXOX...', 'XXOXXXXX', 'XXXXOOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['........', 'OOOOOOO.', 'XOXOX...', 'XXOXXXXX', 'XXXXOOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['..X.....', 'OXXXOOO.', 'XOXOX...', 'XXOXXXXX', 'XXXXOOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['..X.....', 'OXXXOOO.', 'XOXOX.O.', 'XXOXXOXX', 'XXXXOOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['..X.....', 'OXXXXXXX', 'XOXOX.X.', 'XXOXXXXX', 'XXXXXOXO', 'XXXXOXXO', 'XXOOOOX.', '.XOOOXXX'], ['..X.....', 'OXXXXXXX', 'OOXOX.X.', 'OXOXXXXX', 'OXXXXOXO', 'OXXXOXXO', 'OXOOOOX.', 'OOOOOXXX'], ['..X.....', 'OXXXXXXX', 'OOXOX.X.', 'OXOXXXXX', 'OXXXXOXX', 'OXXXOXXX', 'OXOOOOXX', 'OOOOOXXX'], ['..X.....', 'OXXXXXXX', 'OOXOOOX.', 'OXOXOOXX', 'OXXOXOXX', 'OXOXOXXX', 'OOOOOOXX', 'OOOOOXXX'], ['..X.....', 'OXXXXXXX', 'OOXOOOX.', 'OXOXOOXX', 'OXXOXOXX', 'OXOXOXXX', 'OOOOOOXX', 'OOOOOXXX']]),
    _case('resign_black', 'F', [65], [['........', '........', '........', '...OX...', '...XO...', '........', '........', '........']], -1.0, True, 2),
    _case('resign_white', 'F', [19, 65], [['........', '........', '...X....', '...XX...', '...XO...', '........', '........', '........'], ['........', '........', '...X....', '...XX...', '...XO...', '........', '........', '........']], -1.0, True, 1),
]


def cases(shape):
    return [c for c in CASES if c['shape'] == shape]


def case(shape, name):
    return next(c for c in CASES if c['shape'] == shape and c['name'] == name)


def board_array(rows_text):
    return np.array([['.XO'.index(ch) for ch in row] for row in rows_text], np.int8)


def board_text(board):
    return [''.join('.XO'[v] for v in row) for row in np.asarray(board)]


def start_board(rows, cols):
    b = np.zeros((rows, cols), np.int8)
    r0, c0 = rows // 2 - 1, cols // 2 - 1
    b[r0, c0] = b[r0 + 1, c0 + 1] = 2
    b[r0, c0 + 1] = b[r0 + 1, c0] = 1
    return b


def ray(board, r, c, d):
    """The cells from (r, c) exclusive in direction d to the board's edge, as a list of (value, (r, c))."""
    dr, dc = DIRECTIONS[d]
    out = []
    r, c = r + dr, c + dc
    while 0 <= r < board.shape[0] and 0 <= c < board.shape[1]:
        out.append((int(board[r, c]), (r, c)))
        r, c = r + dr, c + dc
    return out


def flipped_by_direction(before, after, point):
    """{direction: number of stones that changed owner on the ray from `point` in that direction} between two boards."""
    r0, c0 = divmod(point, before.shape[1])
    out = {}
    for d in range(8):
        n = sum(1 for v, (r, c) in ray(before, r0, c0, d) if v != 0 and after[r, c] != v)
        if n:
            out[d] = n
    return out


def observation_from_boards(boards_newest_first, to_play, stack_history, rows, cols):
    """The observation written from board snapshots, not from shifted planes: `boards_newest_first` lists the boards as they stood after
    each ply, newest first, the start position last.  Plane 2k: the stones of the side to move k plies ago; plane 2k + 1: the opponent's;
    the last plane: 1 where black is to move."""
    out = np.zeros((2 * stack_history + 1, rows, cols), np.int8)
    for k in range(min(stack_history, len(boards_newest_first))):
        out[2 * k] = boards_newest_first[k] == to_play
        out[2 * k + 1] = boards_newest_first[k] == 3 - to_play
    out[-1] = 1 if to_play == 1 else 0
    return out


# the directions whose shift moves the column: each has an edge mask of its own
EDGE_DIRECTIONS = tuple(n for d, n in enumerate(DIRECTION_NAMES) if DIRECTIONS[d][1] != 0)
BUGS = ('no_edge_mask',) + tuple('no_edge_mask_' + n for n in EDGE_DIRECTIONS) + tuple('direction_missing_' + n for n in DIRECTION_NAMES) + (
    'flip_without_anchor', 'flip_through_empty', 'pass_beside_placements', 'no_pass', 'end_on_full_board_only', 'winner_is_mover',
    'draw_is_loss', 'count_before_flips', 'mover_history_only', 'mask_wrong_colour', 'switch_after_end', 'mask_stale_after_pass')


class OthModel:
    """The device step of one env, in the kernel's formulation (see the module docstring)."""

    def __init__(self, rows, cols, bug=None):
        assert bug is None or bug in BUGS
        self.rows, self.cols, self.bug = rows, cols, bug
        self.nn, self.A = rows * cols, rows * cols + 2
        self.full = (1 << self.nn) - 1
        self.reach = max(rows, cols) - 2
        col = lambda c: sum(1 << (r * cols + c) for r in range(rows))  # noqa: E731
        self.dirs = []
        for d in range(8):
            k = d & 3
            sh, left = (1 if k == 0 else cols + k - 2), d < 4
            dc = 0 if k == 2 else (-1 if k == 1 else 1) * (1 if left else -1)
            unmasked = bug in ('no_edge_mask', 'no_edge_mask_' + DIRECTION_NAMES[d])
            keep = self.full if dc == 0 or unmasked else self.full & ~col(0 if dc > 0 else cols - 1)
            if bug != 'direction_missing_' + DIRECTION_NAMES[d]:
                self.dirs.append((sh, left, keep))
        self.episodes = 0
        self._fresh()

    def _shift(self, x, D):
        sh, left, keep = D
        return ((x << sh) if left else (x >> sh)) & keep

    def moves(self, mine, theirs):
        out = 0
        for D in self.dirs:
            t = self._shift(mine, D) & theirs
            for _ in range(1, self.reach):
                t |= self._shift(t, D) & theirs
            out |= self._shift(t, D) & ~(mine | theirs)
        return out & self.full

    def flips(self, spot, mine, theirs):
        out = 0
        through = theirs if self.bug != 'flip_through_empty' else self.full & ~mine & ~spot
        for D in self.dirs:
            run = self._shift(spot, D) & through
            for _ in range(1, self.reach):
                run |= self._shift(run, D) & through
            if (self._shift(run, D) & ~run & mine) or (self.bug == 'flip_without_anchor' and run):
                out |= run & theirs
        return out

    def _bits(self, x):
        return ((np.uint64(x) >> np.arange(self.nn, dtype=np.uint64)) & np.uint64(1)).astype(np.int8)

    def _set_mask(self, moves):
        self.mask = np.zeros(self.A, np.uint8)
        self.mask[:self.nn] = self._bits(moves)
        self.mask[self.nn] = 0 if self.bug == 'no_pass' else (1 if moves == 0 or self.bug == 'pass_beside_placements' else 0)
        self.mask[self.nn + 1] = 1

    def _fresh(self):
        self.board = start_board(self.rows, self.cols).reshape(-1)
        black = sum(1 << int(i) for i in np.flatnonzero(self.board == 1))
        white = sum(1 << int(i) for i in np.flatnonzero(self.board == 2))
        self.planes = np.zeros((2, 4, self.nn), np.int8)
        self.planes[0, 0], self.planes[1, 0] = self._bits(black), self._bits(white)
        self.player, self.steps = 1, 0
        self._set_mask(self.moves(black, white))
        self.obs = np.zeros((9, self.nn), np.float32)
        self.obs[0], self.obs[1], self.obs[8] = self.planes[0, 0], self.planes[1, 0], 1.0

    def step(self, a):
        """Returns dict(reward, done, winner, board: the position after the move and before any reset, to_play: the side to move
        after the move and before any reset)."""
        nn = self.nn
        me, opp, st = self.player, 3 - self.player, self.steps
        stones = {1: sum(1 << int(i) for i in np.flatnonzero(self.board == 1)), 2: sum(1 << int(i) for i in np.flatnonzero(self.board == 2))}
        before = dict(stones)
        winner, reward, done = 0, 0.0, False
        if a > nn:
            reward, winner, done = -1.0, opp, True
        elif a < nn:
            spot = 1 << a
            f = self.flips(spot, stones[me], stones[opp])
            stones[me] |= spot | f
            stones[opp] &= ~f
        moves = {1: self.moves(stones[1], stones[2]), 2: self.moves(stones[2], stones[1])}
        if a < nn:
            over = (moves[1] | moves[2]) == 0
            if self.bug == 'end_on_full_board_only':
                over = (stones[1] | stones[2]) == self.full
            if over:
                counted = before if self.bug == 'count_before_flips' else stones
                mine, theirs = bin(counted[me]).count('1'), bin(counted[opp]).count('1')
                done = True
                if self.bug == 'winner_is_mover':
                    reward, winner = 1.0, me
                elif mine > theirs:
                    reward, winner = 1.0, me
                elif mine < theirs or self.bug == 'draw_is_loss':
                    reward, winner = -1.0, opp
        after = (self._bits(stones[1]) + 2 * self._bits(stones[2])).astype(np.int8)
        out = dict(reward=reward, done=done, winner=winner or None, board=after.reshape(self.rows, self.cols),
                   to_play=me if done and self.bug != 'switch_after_end' else opp)
        if not done:
            for p in (1, 2):
                if self.bug == 'mover_history_only' and p != me:
                    continue
                hist = self.planes[p - 1]
                hist[1:] = hist[:-1].copy()
                hist[0] = self._bits(stones[p])
            self.board = after
            self.player, self.steps = opp, st + 1
            if not (self.bug == 'mask_stale_after_pass' and a == nn):
                self._set_mask(moves[me if self.bug == 'mask_wrong_colour' else opp])
            self.obs[0:8:2] = self.planes[opp - 1]
            self.obs[1:8:2] = self.planes[me - 1]
            self.obs[8] = 1.0 if opp == 1 else 0.0
        else:
            self.episodes += 1
            self._fresh()
        self.last = out
        return out


def make_env(shape, stack_history=4):
    from muzero_amd.games import OthelloEnv

    rows, cols = SHAPES[shape]
    return OthelloEnv(rows, cols, stack_history)


def model_vs_env(model, env, moves):
    """Steps both; returns the first difference as a string, or None.  After a finished game the env is reset, as the device resets."""
    for ply, a in enumerate(moves):
        mover = env.current_player
        try:
            obs, reward, done, _ = env.step(a)
        except ValueError:
            return f'ply {ply}: the env refuses action {a}'
        out = model.step(a)
        if out['reward'] != reward or out['done'] != done or out['winner'] != env.winner:
            return f'ply {ply}: reward / done / winner {out["reward"], out["done"], out["winner"]} != {reward, done, env.winner}'
        if not np.array_equal(out['board'], env.board):
            return f'ply {ply}: board'
        if out['to_play'] != env.current_player or (done and env.current_player != mover):
            return f'ply {ply}: side to move'
        if done:
            obs = env.reset()
        if model.player != env.current_player or model.steps != env.steps:
            return f'ply {ply}: player / steps after the move'
        if not np.array_equal(model.mask, env.actions_mask.astype(np.uint8)):
            return f'ply {ply}: mask'
        if not np.array_equal(model.obs.reshape(obs.shape), obs.astype(np.float32)):
            return f'ply {ply}: observation'
        if not np.array_equal(model.board.reshape(env.board.shape), env.board):
            return f'ply {ply}: board after the move'
        for pid in (1, 2):
            if not np.array_equal(model.planes[pid - 1].reshape(env.feature_planes[pid].shape), env.feature_planes[pid]):
                return f'ply {ply}: history planes'
    return None
