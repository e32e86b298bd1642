"""The cases of tests/test_gpu_correlate_stack.py, kept here so that tests/test_correlate_stack_host.py can hold the model and the CPU
path to the same ones."""
import functools

import numpy as np

import correlate_stack_model as csm

SHAPES = {
    'small': (5, 19, 37),          # one piece per patch
    'pieces': (2, 97, 150),        # the (1, 1) patch spans 2 x 3 pieces of 64 x 64
    'flat': (3, 1, 23),            # an extent of 1 on either axis
    'thin': (3, 23, 1),
}
assert csm.plan(97, 150, (0, 0), (1, 1))['pieces_y'] == 2 and csm.plan(97, 150, (0, 0), (1, 1))['pieces_x'] == 3
assert csm.plan(19, 37, (0, 0), (1, 1))['pieces'] == 1


@functools.lru_cache(maxsize=None)
def stack(name, integers=False):
    rng = np.random.default_rng(sorted(SHAPES).index(name) + (100 if integers else 0))
    if integers:
        return rng.integers(-8, 9, SHAPES[name]).astype(np.float32)
    return rng.standard_normal(SHAPES[name]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def references(name, n, integers=False):
    """(n, H, W) float32 references for the stack."""
    rng = np.random.default_rng(1000 + sorted(SHAPES).index(name) + (100 if integers else 0))
    shape = (n,) + SHAPES[name][1:]
    if integers:
        return rng.integers(-8, 9, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def case(name, stack_name, max_shift, grid, ref='shared', planes=None, ref_planes=None):
    return dict(name=name, stack=stack_name, max_shift=max_shift, grid=grid, ref=ref, planes=planes, ref_planes=ref_planes)


def arguments(c, integers=False):
    """(stack, references or None, keyword arguments) of a case."""
    s = stack(c['stack'], integers)
    n = len(c['planes']) if c['planes'] is not None else s.shape[0]
    if c['ref'] == 'shared':
        refs = references(c['stack'], 1, integers)[0]
    elif c['ref'] == 'own':
        refs = references(c['stack'], n, integers)
    else:
        refs = None
    kw = dict(planes=c['planes'])
    if c['ref'] == 'resident':
        kw['reference_planes'] = c['ref_planes']
    return s, refs, kw


def _edge_cases():
    out = []
    H, W = SHAPES['pieces'][1:]
    for rw in csm.block_edges_v(60):                         # both sides of every column-block edge below 60
        for r in (rw, rw + 1):
            out.append(case(f'pieces-v-edge-{r}', 'pieces', (1, r), (1, 1), 'shared', [1]))
    for rh, rw in csm.block_edges_u(40, 60):                 # for every count of runs: one row block exactly, and two
        for r in (rh, rh + 1):
            out.append(case(f'pieces-u-edge-{r}-{rw}', 'pieces', (r, rw), (1, 1), 'shared', [0]))
    return out


CASES = [
    # windows on the one-piece stack
    case('small-r00', 'small', (0, 0), (1, 1)),
    case('small-r10', 'small', (1, 0), (1, 1)),
    case('small-r01', 'small', (0, 1), (1, 1)),
    case('small-r27', 'small', (2, 7), (1, 1), 'own'),
    case('small-full', 'small', (18, 36), (1, 1), 'own', [3, 0]),
    # grids
    case('small-g35', 'small', (2, 7), (3, 5), 'own'),
    case('small-gH1', 'small', (1, 2), (19, 1)),
    case('small-g1W', 'small', (2, 1), (1, 37)),
    case('small-gHW', 'small', (1, 1), (19, 37), 'shared', [2]),
    # references shared, per entry, resident; repeated and permuted planes
    case('small-repeat', 'small', (2, 3), (2, 2), 'own', [4, 4, 0, 2, 0, 1, 3]),
    case('small-resident', 'small', (3, 2), (2, 3), 'resident', [1, 2, 3, 4, 0, 2], [0, 1, 2, 3, 4, 2]),
    case('small-resident-all', 'small', (1, 1), (1, 1), 'resident', None, [1, 2, 3, 4, 0]),
    # several pieces per patch, on both axes; uneven patches over pieces
    case('pieces-r00', 'pieces', (0, 0), (1, 1)),
    case('pieces-r27', 'pieces', (2, 7), (1, 1), 'own'),
    case('pieces-g12', 'pieces', (3, 3), (1, 2), 'resident', [0, 1], [1, 0]),       # patches of 75 columns: two pieces, the second 11 wide
    case('pieces-g35', 'pieces', (4, 2), (3, 5), 'shared'),
    # extents of 1
    case('flat-r0-5', 'flat', (0, 5), (1, 1)),
    case('flat-full', 'flat', (0, 22), (1, 3), 'own'),
    case('thin-r5-0', 'thin', (5, 0), (1, 1)),
    case('thin-full', 'thin', (22, 0), (4, 1), 'resident', [0, 1, 2], [2, 2, 0]),
] + _edge_cases()

assert len({c['name'] for c in CASES}) == len(CASES)
