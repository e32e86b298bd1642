"""The weight matrices of tests/test_gpu_warp_stack_sum.py and tests/test_warp_stack_sum_host.py for the n = 10 entries of
tests/warp_stack_cases.py, kept apart so that both files see the same columns.  Numpy only."""
import numpy as np

import warp_stack_cases as wc

N = wc.N
GC = 4                                  # the kernel's chunk of columns (kWarpStackSumChunk)
G_VALUES = (1, 2, GC, GC + 1, 2 * GC + 1)
INSIDE = 1                              # an entry whose image covers most of the output
LAST = N - 1
ONE_HOT_WEIGHT = -1.5


def one_hot(k, w=ONE_HOT_WEIGHT):
    c = np.zeros(N)
    c[k] = w
    return c


def _parity(first):
    c = np.zeros(N)
    c[first::2] = 1.0
    return c


# name -> column; the order is the order of matrix(9)
COLUMNS = {
    'ones': np.ones(N),
    'mixed': np.array(wc.WEIGHTS),                    # mixed signs, one exact 0
    'zero': np.zeros(N),
    'hot_inside': one_hot(INSIDE),
    'hot_outside': one_hot(wc.OUTSIDE),               # the entry that maps wholly outside the image
    'hot_last': one_hot(LAST),
    'even': _parity(0),
    'odd': _parity(1),
    'ramp': np.linspace(-0.9, 1.35, N),               # no zero, no repeat
}
NAMES = tuple(COLUMNS)
assert len(NAMES) == max(G_VALUES)


def matrix(names):
    """(n, G) float64, C order, of the named columns."""
    return np.ascontiguousarray(np.stack([COLUMNS[k] for k in names], axis=1))


def first(g):
    """The first g columns: G_VALUES cross the chunk edges at GC and 2 GC."""
    return NAMES[:g], matrix(NAMES[:g])


def placements():
    """(names, matrix) such that every column appears in every position of a chunk and in more than one chunk: the rotations of NAMES by
    0, 1, 2 and 5, each at G = 9, and the reversed order at G = GC + 1."""
    for r in (0, 1, 2, 5):
        names = NAMES[r:] + NAMES[:r]
        yield names, matrix(names)
    names = NAMES[::-1][:GC + 1]
    yield names, matrix(names)
