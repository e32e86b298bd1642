"""The cases of tests/test_warp_host.py and tests/test_gpu_warp.py: one source shape, the outputs that cut every tile of the family,
affine fields (grids whose interpolation is an affine map again, so the oracle of `extract` applies) and fields that are not affine."""
import functools

import numpy as np

import warp_model as wm

SRC = (40, 44, 52)
OUT_A, OUT_B, OUT_C = (10, 18, 18), (10, 26, 18), (24, 40, 48)
# linear tiles (8, 8, 16) / (8, 16, 16), cubic (8, 8, 16): every output is cut in every dimension
# A (3, 5, 4) grid has integer node spacing on none of the three outputs above (o - 1 = 9, 17, 17 / 9, 25, 17 / 23, 39, 47), and only
# nodes at dyadic coordinates hold an affine field exactly in float32: that grid gets an output of its own, cut in every dimension too.
OUT_354 = (9, 17, 19)
INTERPS = ('linear', 'bspline', 'bspline_simple', 'filt_bspline', 'filt_bspline_simple')


@functools.lru_cache(maxsize=None)
def source_volume():
    vol = np.random.RandomState(2020).random_sample(SRC).astype(np.float32)
    vol.setflags(write=False)
    return vol


def nodes(grid_shape, out_shape):
    """Output coordinates of the nodes, float64 (gD, gH, gW, 3); an axis of one node sits in the middle (utils.grid_nodes' convention,
    written out here on its own)."""
    ax = [np.array([(o - 1) / 2.0]) if g == 1 else np.arange(g, dtype=np.float64) * (o - 1) / (g - 1) for g, o in zip(grid_shape, out_shape)]
    n = np.empty(tuple(grid_shape) + (3,), np.float64)
    n[..., 0], n[..., 1], n[..., 2] = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    return n


def rotated(out_shape, angles=(7.0, -11.0, 5.0), scale=1.0, shift=(0.137, -0.291, 0.213)):
    """A pull matrix, float64: a rotation about the centres (output centre -> source centre) with a translation that is not dyadic."""
    import voltools_amd as vt
    R = vt.utils.rotation_matrix(angles, 'deg', 'sxyz', dtype=np.float64)[:3, :3] * scale
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = (np.asarray(SRC, np.float64) - 1) / 2 + np.asarray(shift) / 3.0 - R @ ((np.asarray(out_shape, np.float64) - 1) / 2)
    return m


# ---- affine fields: u(x) = B x + c with dyadic B, c on nodes at integer output coordinates ----
B_DYADIC = np.array([[0.125, -0.0625, 0.03125], [0.0625, 0.25, -0.125], [-0.03125, 0.0625, 0.1875]])
C_DYADIC = np.array([0.75, -1.5, 0.625])


def affine_field_cases():
    """(name, out_shape, grid float32, B, c)"""
    out = []
    for name, g, o in (('g222', (2, 2, 2), OUT_A), ('g222b', (2, 2, 2), OUT_B), ('g354', (3, 5, 4), OUT_354), ('dense', OUT_A, OUT_A),
                       ('denseC', OUT_C, OUT_C)):
        n = nodes(g, o)
        assert np.array_equal(n, np.round(n)), name                      # node spacing divides o - 1
        field = n @ B_DYADIC.T + C_DYADIC
        grid = field.astype(np.float32)
        assert np.array_equal(grid.astype(np.float64), field), name      # exact in float32
        out.append((name, o, grid, B_DYADIC, C_DYADIC))
    out.append(('zero111', OUT_A, np.zeros((1, 1, 1, 3), np.float32), np.zeros((3, 3)), np.zeros(3)))
    return out


def combined(m, B, c):
    """M + [B | c]"""
    t = np.array(m, np.float64)
    t[:3, :3] += B
    t[:3, 3] += c
    return t


# ---- fields that are not affine ----
def _random_grid(g, amp, seed):
    return np.random.RandomState(seed).uniform(-amp, amp, tuple(g) + (3,)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def field_cases():
    """name -> (out_shape, grid float32, matrix float64)"""
    cases = {
        'g222_a1.5': (OUT_A, _random_grid((2, 2, 2), 1.5, 1), rotated(OUT_A)),
        'g345_a12': (OUT_B, _random_grid((3, 4, 5), 12.0, 2), rotated(OUT_B)),
        'g4x1x6_a1.5': (OUT_B, _random_grid((4, 1, 6), 1.5, 3), rotated(OUT_B, (3.0, 9.0, -14.0))),
        'dense_a1.5': (OUT_A, _random_grid(OUT_A, 1.5, 4), rotated(OUT_A, (-5.0, 4.0, 12.0))),
        'g467_a12': (OUT_C, _random_grid((4, 6, 7), 12.0, 5), rotated(OUT_C, (4.0, -6.0, 3.0))),
        'g12x20x24_a1.5': (OUT_C, _random_grid((12, 20, 24), 1.5, 6), rotated(OUT_C, (20.0, 30.0, -25.0))),
    }
    spike = _random_grid((4, 6, 7), 1.5, 7)
    spike[1, 2, 3, 1] = 200.0                                            # one node, one component: its cells' tiles leave the cap
    cases['spike200'] = (OUT_C, spike, rotated(OUT_C, (2.0, 3.0, -4.0)))
    # the low-w third of the output is pushed far below axis 2's lower face: a face region and whole tiles end up outside
    push = _random_grid((2, 2, 4), 1.5, 8)
    push[:, :, 0, 2] -= 90.0
    push[:, :, 1, 2] -= 30.0
    cases['pushed_out'] = (OUT_C, push, rotated(OUT_C, (1.0, -2.0, 2.0)))
    return cases


@functools.lru_cache(maxsize=None)
def model_result(name, interp):
    """(values float64, inside, coords, plan) of a field case, computed once per session."""
    out_shape, grid, m = field_cases()[name]
    vals, ins, s = wm.warp(source_volume(), m, grid, out_shape, interp)
    for a in (vals, ins, s):
        a.setflags(write=False)
    return vals, ins, s, wm.plan(m, grid, out_shape, interp)
