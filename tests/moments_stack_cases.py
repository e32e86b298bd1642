"""The cases of tests/test_gpu_moments_stack.py, kept here so that tests/test_moments_stack_host.py can hold the model and the CPU path to
the same ones.  The stacks are tests/correlate_stack_cases.py's."""
import numpy as np

import voltools_amd as vt

import correlate_stack_cases as csc
import moments_stack_model as msm

SHAPES = csc.SHAPES
stack = csc.stack

# the (1, 1) patch of `pieces` is walked in five chunks of 32 columns, the last 22 wide (two whole groups of 8 and a part), in one row
# block or several with the window; `small` in two chunks, the second 5 wide
assert msm.plan(97, 150, (0, 0), (1, 1))['row_blocks'] == 1 and msm.plan(97, 150, (0, 20), (1, 1))['row_blocks'] == 2
assert msm.plan(97, 150, (0, 30), (1, 1))['row_blocks'] == 3 and msm.plan(19, 37, (0, 36), (1, 1))['row_blocks'] == 1


def case(name, stack_name, max_shift, grid, planes=None):
    return dict(name=name, stack=stack_name, max_shift=max_shift, grid=grid, planes=planes)


def arguments(c, integers=False):
    """(stack, keyword arguments) of a case."""
    return stack(c['stack'], integers), dict(planes=c['planes'])


def _window_cases():
    """The windows (0, 0), (1, 0), (0, 1), (2, 7) and the full one on every stack, cut to what the stack allows."""
    out = []
    for name in sorted(SHAPES):
        T, H, W = SHAPES[name]
        seen = set()
        for rh, rw in ((0, 0), (1, 0), (0, 1), (2, 7), (H - 1, W - 1)):
            win = (min(rh, H - 1), min(rw, W - 1))
            if win in seen:
                continue
            seen.add(win)
            full = win == (H - 1, W - 1)
            # the full window of `pieces` has 193 x 299 shifts: one image of it
            out.append(case(f'{name}-r{win[0]}-{win[1]}', name, win, (1, 1), [T - 1] if full and name == 'pieces' else None))
    return out


def _grid_cases():
    """The grids (1, 1), (3, 5), (H, 1), (1, W) and (H, W) on every stack, cut to what the stack allows."""
    out = []
    for name in sorted(SHAPES):
        T, H, W = SHAPES[name]
        win = (min(2, H - 1), min(3, W - 1))
        seen = set()
        for gh, gw in ((1, 1), (3, 5), (H, 1), (1, W), (H, W)):
            grid = (min(gh, H), min(gw, W))
            if grid in seen:
                continue
            seen.add(grid)
            many = grid[0] * grid[1] > 1000                     # (H, W) of `pieces`: 14550 patches, one image and a window of (1, 1)
            out.append(case(f'{name}-g{grid[0]}-{grid[1]}', name, (min(1, H - 1), min(1, W - 1)) if many else win, grid, [0] if many else None))
    return out


def _edge_cases():
    """Both sides of every edge of the plan below a window of 60 columns on `pieces`: the count of runs, of row blocks (97 rows against
    256, 128, 84, 64, 48, 40 and 36 per workgroup) and of column-shift blocks."""
    out = []
    H, W = SHAPES['pieces'][1:]
    done = set()
    for rw in msm.plan_edges(H, W, 60):
        for r in (rw, rw + 1):
            if r not in done:
                done.add(r)
                out.append(case(f'pieces-edge-{r}', 'pieces', (1, r), (1, 1), [1]))
    return out


CASES = _window_cases() + _grid_cases() + [
    # repeated and permuted planes
    case('small-repeat', 'small', (2, 3), (2, 2), [4, 4, 0, 2, 0, 1, 3]),
    case('pieces-permuted', 'pieces', (3, 2), (1, 2), [1, 0, 1]),                       # patches of 75 columns: 32 + 32 + 11
    # patches of 16 and 17 columns (two whole groups; two and a part), of 32 and 33 rows
    case('pieces-g3-9', 'pieces', (2, 3), (3, 9)),
    # a tall window over several row blocks and column-shift blocks at once
    case('pieces-r40-45', 'pieces', (40, 45), (2, 3), [0]),
] + _edge_cases()

assert len({c['name'] for c in CASES}) == len(CASES)


# ---- the shift-recovery trials of the host and the GPU tests ---------------------------------------------------------------------------
def bright_series(seed, d, H=60, W=72, pad=16):
    """A reference and one image displaced by the integer d = (dy, dx), image[y + d] == reference[y], cut from a canvas of mean 10
    and unit noise that carries two Gaussian blobs of amplitude 40 and sigma 2 just outside the centre patch of the 3 x 3 grid."""
    rng = np.random.default_rng(seed)
    canvas = 10.0 + rng.standard_normal((H + 2 * pad, W + 2 * pad))
    yy, xx = np.mgrid[0:H + 2 * pad, 0:W + 2 * pad]
    for cy, cx in ((pad + 17, pad + 21), (pad + 44, pad + 52)):
        canvas += 40.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.0 ** 2))
    dy, dx = d
    ref = np.ascontiguousarray(canvas[pad:pad + H, pad:pad + W], dtype=np.float32)
    img = np.ascontiguousarray(canvas[pad - dy:pad - dy + H, pad - dx:pad - dx + W], dtype=np.float32)
    return ref, img


SEEDS, SHIFTS, WINDOW, GRID = range(6), ((3, -2), (-4, 1), (2, 4)), (5, 5), (3, 3)


def recovery(device):
    """The 18 trials: per trial (shift found with normalized=True, with normalized=False, the coefficients) of the centre patch."""
    out = []
    for seed in SEEDS:
        for d in SHIFTS:
            ref, img = bright_series(seed, d)
            sv = vt.StaticVolume(img[None], device=device)
            try:
                fine = sv.find_shifts(ref, WINDOW, GRID, subpixel=False, normalized=True)
                raw = sv.find_shifts(ref, WINDOW, GRID, subpixel=False, normalized=False)
                assert np.array_equal(raw, sv.find_shifts(ref, WINDOW, GRID, subpixel=False))
                ncc = sv.correlate_stack_normalized(ref, WINDOW, GRID)
            finally:
                if device != 'cpu':
                    sv.close()
            out.append((d, fine[0, 1, 1], raw[0, 1, 1], ncc[0, 1, 1]))
    return out


def check_recovery(trials):
    assert len(trials) == 18
    for d, fine, raw, ncc in trials:
        assert tuple(fine) == d, (d, fine)                                               # the coefficient finds the shift exactly
        top = np.sort(ncc.ravel())
        assert abs(top[-1] - 1.0) < 1e-6 and top[-2] <= 0.26, (d, top[-2:])
        assert ncc[d[0] + WINDOW[0], d[1] + WINDOW[1]] == top[-1]
        assert max(abs(raw[0]), abs(raw[1])) == 5 and tuple(raw) != d, (d, raw)          # the raw peak sits on the window's rim
