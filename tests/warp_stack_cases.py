"""The cases of tests/test_gpu_warp_stack.py, kept apart so that tests/test_warp_stack_host.py can hold the model to them without a GPU
(the skirt condition, the plan properties).  Nothing here touches the library beyond utils-free numpy."""
import functools

import numpy as np

import lattice_cases as lc

STACK = (6, 40, 52)
OUT = (37, 45)                         # the (1, 16, 16) tile, cut tiles on both axes
OUT32 = (61, 59)                       # the (1, 32, 32) tile
TILE = {OUT: (1, 16, 16), OUT32: (1, 32, 32)}
PLANES = np.array([0, 5, 2, 2, 3, 1, 4, 0, 5, 3])
WEIGHTS = np.array([0.75, -1.5, 2.0, 0.0, 1.25, -0.5, 1.0, 0.6, 1.5, -2.0])       # mixed signs, one exact 0
NONZERO = np.where(WEIGHTS == 0, 0.5, WEIGHTS)
OUTSIDE = 7
N = 10
GRID_SHAPES = ((2, 2), (3, 5), (1, 4), (4, 1), (1, 1), 'dense')
AMPLITUDES = (1.5, 12.0)


def in_plane(lin, out, at=None, image=STACK):
    """4x4 float64 matrix whose rows 1 and 2 carry the 2 x 2 linear part `lin` in columns 1 and 2 and send the centre of the output image
    to the image point `at` (default: the image centre).  Row 0 and column 0 are junk on purpose: they are ignored."""
    lin = np.asarray(lin, np.float64)
    c = (np.asarray(out, np.float64) - 1) / 2
    at = (np.asarray(image[-2:], np.float64) - 1) / 2 if at is None else np.asarray(at, np.float64)
    m = np.eye(4)
    m[0] = (0.3, -0.7, 0.2, 11.0)
    m[1:3, 0] = (0.25, -0.5)
    m[1:3, 1:3] = lin
    m[1:3, 3] = at - lin @ c
    return m


def rot(deg):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


@functools.lru_cache(maxsize=None)
def batch(out=OUT):
    """Ten float64 matrices in the style of test_gpu_stack_affine.batch(): the identity at a sub-pixel offset, a rotation by 30 degrees, a
    rotation within 1e-3 of 45 degrees, scale 0.5, scale 2, a shear, a sub-pixel shift, one entry wholly outside, two entries partly
    outside.  (No translation is a multiple of 1/8: with random grids no coordinate lands on a skirt face but by chance.)"""
    ident = in_plane(np.eye(2), out)
    ident[1, 3], ident[2, 3] = 3.1, 4.3
    sub = in_plane(np.eye(2), out)
    sub[1, 3], sub[2, 3] = 1.37, 2.81
    ms = [ident, in_plane(rot(30.0), out), in_plane(rot(45.0005), out, (19.25, 26.5)), in_plane(0.5 * np.eye(2), out),
          in_plane(2.0 * np.eye(2), out), in_plane([[1.0, 0.35], [-0.2, 1.0]], out), sub,
          in_plane(np.eye(2), out, (1000.0, -700.0)), in_plane(np.eye(2), out, (35.5, -4.25)), in_plane(1.2 * rot(-70.0), out, (6.0, 44.0))]
    ms = np.ascontiguousarray(np.stack(ms))
    ms.setflags(write=False)
    return ms


def grid_shape(gs, out):
    return tuple(out) if gs == 'dense' else gs


@functools.lru_cache(maxsize=None)
def grids(gs, amp, out=OUT, n=N, seed=5):
    """n random float32 grids of shape gs ('dense': the output's), components uniform in [-amp, amp)."""
    g = grid_shape(gs, out)
    rs = np.random.RandomState(seed + 7 * GRID_SHAPES.index(gs) + int(amp))
    a = ((rs.random_sample((n,) + g + (2,)) * 2.0 - 1.0) * amp).astype(np.float32)
    a.setflags(write=False)
    return a


def parity_cases():
    """(name, out, matrices or None, grids (n, gH, gW, 2)) of the model parity test."""
    for out in (OUT, OUT32):
        for gs in GRID_SHAPES:
            for amp in AMPLITUDES:
                yield f'{out[0]}x{out[1]}-{gs}-{amp}', out, batch(out), grids(gs, amp, out)
        yield f'{out[0]}x{out[1]}-identity', out, None, grids((3, 5), 1.5, out, STACK[0], 9)


# ---- the routes ------------------------------------------------------------------------------------------------------------------------
def spike_case(out=OUT):
    """Entry 1 carries a 200-pixel spike in one node of a (3, 5) grid; its neighbours are calm."""
    g = np.array(grids((3, 5), 1.5, out, 3, 21))
    g[1, 1, 2] = (200.0, -200.0)
    ms = np.stack([batch(out)[0], batch(out)[0], batch(out)[6]])
    return ms, g, np.array([1, 1, 4]), np.array([1.0, -0.5, 2.0])


def hull_case(out=OUT):
    """Nodes of +-2^19 with five nodes on an axis: U (g - 1) = 2^21 > 2^20, the hull is not granted."""
    g = np.zeros((1, 2, 5, 2), np.float32)
    g[0, :, ::2, 1] = 2.0 ** 19
    g[0, :, 1::2, 1] = -2.0 ** 19
    return batch(out)[:1].copy(), g, np.array([2]), np.array([1.0])


def extent_case(out=OUT):
    """A scale of 140: 140 x 15 = 2100 per row term, 4200 >= 4096 with the shear term."""
    m = in_plane([[140.0, 140.0], [0.0, 1.0]], out)
    return m[None].copy(), np.array(grids((2, 2), 1.5, out, 1, 3)), np.array([3]), np.array([1.0])


def chain_case(out=OUT):
    """A translation of 2^25: the chain terms pass 2^24."""
    m = in_plane(np.eye(2), out)
    m[2, 3] = 2.0 ** 25
    g = np.zeros((1, 1, 1, 2), np.float32)
    g[0, 0, 0, 1] = -2.0 ** 25 + 7.3
    return m[None].copy(), g, np.array([0]), np.array([1.0])


def route_cases():
    return {'spike': spike_case(), 'hull': hull_case(), 'extent': extent_case(), 'chain': chain_case()}


# ---- the exact lattice -------------------------------------------------------------------------------------------------------------------
DYADIC = ((0.0, 0.0), (0.5, -0.5), (-0.5, 0.5), (0.25, -0.75), (3.0, -2.0), (1.5, 11.5))


def lattice_case():
    """Integer shifts (the bases of tests/lattice_cases.py) under the identity, one dyadic constant grid per entry: the chain and the
    lerps are exact, y = h + t + c.  With c = +-0.5 whole rows and columns lie exactly on the skirt faces."""
    bases = [lc._base_for(b, STACK[2]) for b in lc.BASES][:len(DYADIC)]
    ms = np.tile(np.eye(4), (len(DYADIC), 1, 1))
    g = np.zeros((len(DYADIC), 2, 3, 2), np.float32)
    for i, (b, c) in enumerate(zip(bases, DYADIC)):
        ms[i, 1, 3], ms[i, 2, 3] = float(b), float(-b)
        g[i] = c
    folded = ms.copy()
    folded[:, 1, 3] += [c[0] for c in DYADIC]
    folded[:, 2, 3] += [c[1] for c in DYADIC]
    return ms, g, folded, np.arange(len(DYADIC))


def pushed_out_case(out=OUT):
    """A (2, 9) grid whose columns 5 .. 8 are pushed 500 pixels out: everything right of w = 27.5 maps beyond the face, and the tiles
    that start at w = 32 see pushed-out nodes only: they are classified wholly outside."""
    g = np.zeros((1, 2, 9, 2), np.float32)
    g[0, :, 5:, 1] = 500.0
    g[0, :, :5, 1] = 0.3
    m = in_plane(np.eye(2), out)
    m[1, 3], m[2, 3] = -3.3, -2.7
    return m[None].copy(), g, np.array([4]), np.array([1.5])


# ---- small and odd shapes ----------------------------------------------------------------------------------------------------------------
# (stack shape, output shape, grid shape): widths 49 - 51, the smallest stacks, outputs of one pixel, one row and one column, a grid of
# the output's shape where an axis has length 2 and where it has one row
SMALL_CASES = [((2, 40, 49), (21, 33), (3, 5)), ((2, 40, 50), (21, 33), (3, 5)), ((2, 40, 51), (21, 33), (21, 33)), ((1, 1, 1), (5, 6), (2, 2)),
               ((1, 2, 3), (5, 6), (5, 6)), ((2, 40, 52), (1, 1), (1, 1)), ((2, 40, 52), (1, 70), (1, 4)), ((2, 40, 52), (70, 1), (4, 1)),
               ((2, 40, 52), (2, 9), (2, 9)), ((2, 40, 52), (9, 2), (9, 2)), ((2, 40, 52), (1, 70), (1, 70))]


def small_case(shape, out, gs):
    """(matrices, grids, planes, weights): the identity, a turn with a magnification and a general map about the image centre (each off
    the lattice by a hundredth of a pixel), grids of amplitude 1.5."""
    ms = np.stack([in_plane(np.eye(2), out, image=shape), in_plane(0.8 * rot(25.0), out, image=shape),
                   in_plane([[0.4, 0.1], [-0.2, 0.7]], out, (shape[1] / 2 - 0.3, shape[2] / 2 + 0.2), image=shape)])
    ms[:, 1:3, 3] += (0.013, 0.029)
    g = ((np.random.RandomState(3).random_sample((3,) + tuple(gs) + (2,)) * 2.0 - 1.0) * 1.5).astype(np.float32)
    return ms, g, np.array([0, shape[0] - 1, 0]), np.array([1.0, -1.5, 0.5])
