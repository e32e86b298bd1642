"""-m gpu: the batched entry points share one handle's scratch -- the host staging vector, the device table, the partial sums and the
result staging buffer -- so a call must not depend on what the call before it left there.  A fixed sequence of affine_batch, extract,
projection_batch, extract_sum, extract_dot, extract_dot_multi, extract_sum_multi, place, backproject and backproject_boxes runs on ONE
handle, each at least twice, ordered so that the table and the partials shrink and grow between neighbours (n = 40 after n = 1, several
segments after one -- box 9 x 13 x 11 has few tiles, so any n > 1 splits --, g = 9 after g = 1, accumulate after a plain call, a host
output after a device output).  Every result must equal, bit for bit, the same call on a fresh handle, and so must the launch record
(last_kernel, last_tile, last_lds, last_lds_bytes, last_grid) of info().

Three handles over a 20 x 22 x 24 volume: linear (the whole sequence), filt_bspline (without the back-projection pair) and filt_bspline
with VT_STACK (the back-projection pair alone)."""
import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

pytestmark = pytest.mark.gpu

SHAPE = (20, 22, 24)
BOX = (9, 13, 11)
OUT = (12, 14, 16)
RNG_SEED = 20


def volume():
    return np.random.RandomState(7).random_sample(SHAPE).astype(np.float32)


def boxes(n, seed, box=BOX):
    """n box matrices, seeded; box 0 hangs over the low face of every axis."""
    rng = np.random.default_rng(RNG_SEED + seed)
    pos = rng.uniform(4.0, 16.0, (n, 3))
    pos[0] = (1.5, 2.25, 0.5)
    return vt.utils.box_matrices(pos, rng.uniform(-180.0, 180.0, (n, 3)), box)


def places(n, seed):
    rng = np.random.default_rng(RNG_SEED + seed)
    pos = rng.uniform(2.0, 11.0, (n, 3))
    pos[0] = (0.5, 13.0, 1.25)                                        # hangs over two faces of the output
    return vt.utils.place_matrices(pos, rng.uniform(-180.0, 180.0, (n, 3)), SHAPE)


def weights(shape, seed):
    return np.random.default_rng(RNG_SEED + seed).uniform(-1.0, 1.0, shape)


def field(shape, seed):
    return np.random.default_rng(RNG_SEED + seed).uniform(-1.0, 1.0, shape).astype(np.float32)


class DeviceF64:
    """A float64 device result (the dot entry points write float64): a float32 DeviceArray of twice the length behind the interface."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.buf = _native.DeviceArray((2 * int(np.prod(shape)),), 0, zero=True)

    @property
    def __cuda_array_interface__(self):
        return {'shape': self.shape, 'typestr': '<f8', 'data': (self.buf.ptr, False), 'version': 2, 'strides': None}

    def get(self):
        return self.buf.get().view(np.float64).reshape(self.shape)


def run(call, shape, device, base=None, f64=False):
    """call(output=...) into a device array or a host array of `shape` (prefilled with `base` for an accumulating call) -> numpy."""
    if device:
        if f64:
            out = DeviceF64(shape)
        else:
            out = _native.DeviceArray.from_numpy(base) if base is not None else _native.DeviceArray(shape, 0, zero=True)
        call(out)
        res = out.get()
        (out.buf if f64 else out).free()
        return res
    out = np.array(base, copy=True) if base is not None else np.full(shape, -7.0, np.float64 if f64 else np.float32)
    call(out)
    return out


def extract(n, seed, device):
    ms = boxes(n, seed)
    return lambda sv: run(lambda o: sv.extract(ms, BOX, output=o), (n,) + BOX, device)


def extract_sum(n, seed, device, w=True):
    ms, ws = boxes(n, seed), weights(n, seed) if w else None
    return lambda sv: run(lambda o: sv.extract_sum(ms, BOX, ws, output=o), BOX, device)


def extract_sum_multi(n, g, seed, device):
    ms, ws = boxes(n, seed), weights((n, g), seed)
    return lambda sv: run(lambda o: sv.extract_sum_multi(ms, BOX, ws, output=o), (g,) + BOX, device)


def extract_dot(n, seed, device, mask=False):
    ms, t, k = boxes(n, seed), field(BOX, seed), np.abs(field(BOX, seed + 1)) if mask else None
    return lambda sv: run(lambda o: sv.extract_dot(ms, t, k, output=o), (n, 3), device, f64=True)


def extract_dot_multi(n, k, seed, device, mask=False):
    ms, t, mk = boxes(n, seed), field((k,) + BOX, seed), np.abs(field(BOX, seed + 1)) if mask else None
    return lambda sv: run(lambda o: sv.extract_dot_multi(ms, t, mk, output=o), (n, 2 + k), device, f64=True)


def projection_batch(n, shape, seed, device):
    ms = vt.utils.tilt_matrices(np.random.default_rng(RNG_SEED + seed).uniform(-60.0, 60.0, n), 1, shape)
    return lambda sv: run(lambda o: sv.projection_batch(ms, shape, output=o), (n,) + tuple(shape[1:]), device)


def affine_batch(n, seed, device):
    rng = np.random.default_rng(RNG_SEED + seed)
    center = np.divide(np.subtract(SHAPE, 1), 2, dtype=np.float32)
    ms = np.stack([vt.utils.transform_matrix(rotation=tuple(rng.uniform(-180.0, 180.0, 3)), rotation_order='rzxz',
                                             translation=tuple(rng.uniform(-2.0, 2.0, 3)), center=center) for _ in range(n)])
    return lambda sv: run(lambda o: sv.affine_batch(ms, output=o), (n,) + SHAPE, device)


def place(n, seed, device, accumulate=False, outside=False):
    ms, ws = places(n, seed), weights(n, seed)
    if outside:                                                       # no copy can land anywhere: with accumulate nothing is launched
        ms = ms.copy()
        ms[:, :3, 3] += 1000.0
    base = field(OUT, seed + 2) if accumulate else None
    return lambda sv: run(lambda o: sv.place(ms, OUT, ws, output=o, accumulate=accumulate), OUT, device, base)


def backproject(n, seed, device, accumulate=False):
    rng = np.random.default_rng(RNG_SEED + seed)
    ms = vt.utils.backproject_matrices(rng.uniform(-60.0, 60.0, n), 1, OUT, SHAPE)
    planes = None if n == SHAPE[0] else rng.integers(0, SHAPE[0], n)
    ws, base = weights(n, seed), field(OUT, seed + 2) if accumulate else None
    return lambda sv: run(lambda o: sv.backproject(ms, OUT, ws, output=o, planes=planes, accumulate=accumulate), OUT, device, base)


def backproject_boxes(nb, n, seed, device, accumulate=False):
    rng = np.random.default_rng(RNG_SEED + seed)
    ms = np.stack([vt.utils.backproject_matrices(rng.uniform(-60.0, 60.0, n), 1, BOX, SHAPE) for _ in range(nb)])
    ms[:, :, 1:3, 3] += rng.uniform(-6.0, 6.0, (nb, 1, 2))
    ms[0, :, 1:3, 3] -= 9.0                                           # box 0 hangs over the images' low edges
    planes = rng.integers(0, SHAPE[0], n)
    ws, base = weights((nb, n), seed), field((nb,) + BOX, seed + 2) if accumulate else None
    return lambda sv: run(lambda o: sv.backproject_boxes(ms, BOX, ws, output=o, planes=planes, accumulate=accumulate),
                          (nb,) + BOX, device, base)


DEV, HOST = True, False
BACK = [
    ('backproject n=20 device', backproject(20, 40, DEV)),
    ('backproject n=6 accumulate host', backproject(6, 41, HOST, accumulate=True)),
    ('backproject_boxes 1x6 device', backproject_boxes(1, 6, 42, DEV)),
    ('backproject_boxes 5x6 accumulate host', backproject_boxes(5, 6, 43, HOST, accumulate=True)),
    ('backproject n=1 device', backproject(1, 44, DEV)),
    ('backproject_boxes 2x3 host', backproject_boxes(2, 3, 45, HOST)),
]
THREE_D = [
    ('extract n=1 device', extract(1, 1, DEV)),
    ('extract n=40 host', extract(40, 2, HOST)),
    ('extract_sum n=1 device', extract_sum(1, 3, DEV, w=False)),
    ('extract_sum n=40 host', extract_sum(40, 4, HOST)),
    ('extract_sum_multi n=5 g=1 device', extract_sum_multi(5, 1, 5, DEV)),
    ('extract_sum_multi n=12 g=9 host', extract_sum_multi(12, 9, 6, HOST)),
    ('extract_dot n=1 device', extract_dot(1, 7, DEV)),
    ('extract_dot n=40 mask host', extract_dot(40, 8, HOST, mask=True)),
    ('extract_dot_multi n=3 k=2 device', extract_dot_multi(3, 2, 9, DEV)),
    ('extract_dot_multi n=17 k=5 mask host', extract_dot_multi(17, 5, 10, HOST, mask=True)),
    ('projection_batch n=1 device', projection_batch(1, (10, 12, 14), 11, DEV)),
    ('projection_batch n=7 host', projection_batch(7, SHAPE, 12, HOST)),
    ('place n=1 device', place(1, 13, DEV)),
    ('place n=9 accumulate host', place(9, 14, HOST, accumulate=True)),
    ('affine_batch n=1 device', affine_batch(1, 15, DEV)),
    ('affine_batch n=3 host', affine_batch(3, 16, HOST)),
    ('extract n=2 device', extract(2, 17, DEV)),
    ('extract_sum n=1 host', extract_sum(1, 18, HOST)),
    ('place outside accumulate host', place(3, 19, HOST, accumulate=True, outside=True)),
    ('extract_sum_multi n=40 g=1 device', extract_sum_multi(40, 1, 20, DEV)),
    ('extract_dot n=2 host', extract_dot(2, 21, HOST)),
    ('place n=9 device', place(9, 22, DEV)),
    ('extract_dot_multi n=1 k=1 host', extract_dot_multi(1, 1, 23, HOST)),
    ('extract_sum n=7 device', extract_sum(7, 24, DEV)),
]
# the back-projection pair between the three-dimensional calls, not behind them
LINEAR = THREE_D[:4] + BACK[:2] + THREE_D[4:10] + BACK[2:4] + THREE_D[10:] + BACK[4:]


def record(sv):
    i = sv.info()
    return (i.last_kernel, tuple(i.last_tile), tuple(i.last_lds_dims), i.last_lds_bytes, i.last_grid)


@pytest.mark.parametrize('interp,stack,steps', [('linear', False, LINEAR), ('filt_bspline', False, THREE_D), ('filt_bspline', True, BACK)],
                         ids=['linear', 'filt_bspline', 'filt_bspline_stack'])
def test_a_call_does_not_depend_on_the_calls_before_it(interp, stack, steps):
    vol = volume()
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', stack=stack)
    try:
        for name, step in steps:
            got, got_rec = step(sv), record(sv)
            fresh = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', stack=stack)
            try:
                want, want_rec = step(fresh), record(fresh)
            finally:
                fresh.close()
            assert got.shape == want.shape and got.dtype == want.dtype, name
            assert np.array_equal(got, want) and np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
            assert got_rec == want_rec, (name, got_rec, want_rec)
            assert np.isfinite(got).all() and (got != -7.0).any(), name              # the call wrote its output
    finally:
        sv.close()
