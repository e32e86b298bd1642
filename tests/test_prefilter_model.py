"""The host model of the prefilter (tests/prefilter_model.py): its float64 recursion against the hand formula and scipy, its constants
against the sources, and the case lists of tests/test_gpu_prefilter.py routed through its dispatch -- every kernel form and every listed
branch must be reached by a case.  CPU only (runs under -m "not gpu")."""
import os
import re

import numpy as np

from oracle import oracle
import prefilter_model as pm
import test_gpu_prefilter as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'voltools_amd', 'csrc')


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
def test_f64_line_equals_the_hand_formula():
    """The formula of tests/test_oracle.py::test_prefilter_line_reference_formula, sample by sample."""
    z = np.sqrt(3.0) - 2.0
    lam = (1 - z) * (1 - 1 / z)
    for n in (1, 2, 5, 12, 13, 40):
        s = np.random.RandomState(n).random_sample(n)
        c = s.copy()
        c[0] = lam * (s[0] + sum(z ** (k + 1) * s[k] for k in range(min(12, n))))
        for k in range(1, n):
            c[k] = lam * s[k] + z * c[k - 1]
        c[n - 1] = z / (z - 1) * c[n - 1]
        for k in range(n - 2, -1, -1):
            c[k] = z * (c[k + 1] - c[k])
        assert np.abs(pm.prefilter_f64(s) - c).max() <= 1e-14 * np.abs(c).max(), n
        # a volume whose only long axis is the line gives the same line (the other axes have one sample: factor (lambda (1 + z) z / (z - 1))^2)
        one = lam * (1 + z) * z / (z - 1)
        assert np.abs(pm.prefilter_f64(s.reshape(1, 1, n))[0, 0] - one * one * c).max() <= 1e-13 * np.abs(c).max(), n
    # the steady-state start: a constant stays constant from the first plane on
    c = pm.prefilter_f64(np.full((40, 1, 1), 2.5), lo_interior_axis0=True)[:, 0, 0] / (one * one)
    assert np.abs(c[:20] - 2.5).max() <= 1e-13


def test_f64_equals_scipy_away_from_the_faces():
    """scipy's spline_filter (mirror boundary, float64) is the same filter with another boundary treatment: 24 samples from every
    face the two boundary terms have decayed to |z|^24 = 2e-14."""
    from scipy import ndimage
    vol = np.random.RandomState(3).random_sample((60, 58, 62))
    got = pm.prefilter_f64(vol)
    want = ndimage.spline_filter(vol, order=3, mode='mirror', output=np.float64)
    inner = (slice(24, -24),) * 3
    rel = np.abs(got[inner] - want[inner]).max() / np.abs(want[inner]).max()
    print(f'prefilter_f64 against scipy, 24 samples from every face: {rel:.2e} relative')
    assert rel <= 1e-12


# ---------------------------------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------------------------------
def test_model_constants_are_the_sources():
    src = read('vt_kernels_prefilter.hip')

    def one(pattern, text=src):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]

    assert tuple(map(int, one(r'constexpr int kChunk = (\d+), kWarm = (\d+);'))) == (pm.K_CHUNK, pm.K_WARM)
    assert int(one(r'constexpr int kBlkK = (\d+);')) == pm.BLK_K
    assert tuple(map(int, one(r'constexpr int kXyNW = (\d+), kXyCW = (\d+), kXyK = (\d+);'))) == (pm.XY_NW, pm.XY_CW, pm.XY_K)
    assert int(one(r'constexpr int kXyCols = (\d+),')) == pm.XY_COLS
    assert one(r'kXyRows = ([^,]+), kXyNetRows = ([^;]+);') == ('kXyNW * kXyCW', 'kXyRows - 2 * kXyK')
    assert one(r'kXyNetCols = ([^;]+);') == 'kXyCols - 2 * kXyK'
    # block variants: VT_PF_BLOCK 1, 2 and the default
    assert tuple(map(int, one(r'blk_variant == 1\) return launch\(prefilter_block<(\d+), (\d+)>'))) == pm.BLK_VARIANTS[1]
    assert tuple(map(int, one(r'blk_variant == 2\) return launch\(prefilter_block<(\d+), (\d+)>'))) == pm.BLK_VARIANTS[2]
    assert tuple(map(int, one(r'\n        return launch\(prefilter_block<(\d+), (\d+)>'))) == pm.BLK_VARIANTS[0]
    assert one(r'const int seg = (nw[^;]+);') == 'nw * cw - 2 * kBlkK'
    assert int(one(r'\(axis == 1 \? H : D\) >= (\d+)\)')) == pm.BLK_MIN_N
    # thresholds
    assert tuple(map(int, one(r'!off && W >= (\d+) && H >= (\d+) &&'))) == (pm.XY_MIN_W, pm.XY_MIN_H)
    assert int(one(r'if \(axis == 2\) return W <= (\d+);')) == pm.X_REG_MAX_W
    assert set(map(int, re.findall(r'axis == 2 && W <= (\d+)', src))) == {pm.X_REG_MAX_W}
    assert int(one(r'return N <= (\d+);')) == pm.IN_PLACE_MAX_N
    assert tuple(map(int, one(r'env_int\("VT_PF_CHUNK", N >= (\d+) \? (\d+) : (\d+)\)'))) == (pm.CHUNK_128_FROM, 128, pm.K_CHUNK)
    assert one(r'return \(variant == 128\) \? 128 : \(variant == 32 \? 32 : (\w+)\);') == 'kChunk'
    assert one(r'const int nsegY = ([^;]+);') == '(H <= kXyRows) ? 1 : (H + kXyNetRows - 1) / kXyNetRows'
    assert one(r'const int nsegX = ([^;]+);') == '(W <= kXyCols) ? 1 : (W + kXyNetCols - 1) / kXyNetCols'
    assert tuple(map(int, one(r'const int nseg = \(W \+ (\d+)\) / (\d+);\s*const dim3 g\(\(unsigned\)blocks\), b\(256\);\s*const int li[^\n]*\n\s*if \(nseg <= 1\) hipLaunchKernelGGL\(prefilter_x_scan4<'))) == (255, 256)
    assert tuple(map(int, one(r'const int nseg = \(W \+ (\d+)\) / (\d+);\s*const dim3 g\(\(unsigned\)blocks\), b\(256\);\s*const int li[^\n]*\n\s*if \(nseg <= 1\) hipLaunchKernelGGL\(prefilter_x_scan<'))) == (63, 64)
    assert int(one(r'const int horizon = W < (\d+) \? W : \1;\s*const float term')) == pm.HORIZON
    # the instantiations the dispatch names
    assert tuple(sorted(set(map(int, re.findall(r'hipLaunchKernelGGL\(prefilter_x_scan<(\d+)>', src))))) == pm.X_SCAN_NSEG
    assert tuple(sorted(set(map(int, re.findall(r'hipLaunchKernelGGL\(prefilter_x_scan4<(\d+)>', src))))) == pm.X_SCAN4_NSEG
    assert set(re.findall(r'prefilter_chunked<(\w+), kWarm>', src)) == {'128', '32', 'kChunk'} and pm.CHUNK_SIZES == (32, 64, 128)
    assert one(r'\(prefilter_xy<(\w+), (\w+)>\)') == ('kXyNW', 'kXyCW')
    assert set(re.findall(r'getenv\("(VT_PF_\w+)"\)|env_int\("(VT_PF_\w+)"', src)) == {('VT_PF_NO_XY', ''), ('VT_PF_NO_BLOCK', ''),
                                                                                       ('', 'VT_PF_CHUNK'), ('', 'VT_PF_BLOCK')}
    # the resident pitch and the one-shot pipeline's thresholds
    host = read('vt_host.h')
    assert one(r'inline int resident_pitch\(int W\) \{ return ([^;]+); \}', host) == '(W + 4 + 31) & ~31'
    assert [pm.resident_pitch(w) for w in (1, 28, 29, 60, 61, 600)] == [32, 32, 64, 64, 96, 608]
    api = read('vt_api.hip')
    assert one(r'n \* sizeof\(float\) < \(\(size_t\)(\d+) << 20\) \|\| D < (\d+)\)', api) == ('32', '32')
    assert pm.ONESHOT_MIN_BYTES == 32 << 20
    assert one(r'const int order\[3\] = \{([^}]+)\};', api) == '2, 1, 0'


# ---------------------------------------------------------------------------------------------------
# coverage of the case lists
# ---------------------------------------------------------------------------------------------------
def routed_cases():
    """(label, Route) of every case the GPU suite runs with no knob set."""
    out = [(f'dense {fam} {shape}', pm.route_dense(shape)) for fam, shape in gp.CASES]
    out += [(f'resident {shape}', pm.route_resident(shape)) for shape in gp.RESIDENT + [gp.RECYCLED]]
    out += [(f'slab depth {d}', pm.route_resident((d, gp.SLAB_H, gp.SLAB_W), lo_interior=True)) for d in gp.SLAB_DEPTHS]
    return out


def test_case_list_reaches_every_form_and_branch():
    rows = {f'{f}<{p}>': [] for f, p in pm.all_default_forms()}
    # (x_scan serves rows that are not whole vectors: with aligned buffers its last segment is never full)
    for name in ('x_scan one segment', 'x_scan ragged last segment',
                 'x_scan4 one segment', 'x_scan4 ragged last segment', 'x_scan4 full last segment',
                 'chunked one chunk', 'chunked ragged last chunk', 'chunked last chunk below the warm-up', 'chunked in place', 'chunked ping-pong',
                 'chunked axis 0', 'chunked axis 1', 'chunked axis 2', 'chunked two lane blocks', 'chunked<128> axis 0', 'chunked<128> axis 1',
                 'chunked line shorter than the horizon',
                 'block one segment', 'block ragged last segment', 'block last segment below the warm-up', 'block axis 0', 'block axis 1',
                 'block one column block', 'block two column blocks', 'block W%4=0', 'block W%4=1', 'block W%4=2', 'block W%4=3',
                 'xy one row segment', 'xy ragged last row segment', 'xy last row segment below the warm-up', 'xy rows at the tile edge',
                 'xy one column segment', 'xy ragged last column segment', 'xy last column segment below the warm-up',
                 'xy W%8=0 dense', 'xy W%4!=0 pitched',
                 'result in the caller\'s buffer (dense)', 'result in the partner buffer (dense: copy back)',
                 'result in the handle\'s buffer (resident)', 'result in the partner buffer (resident: swap)',
                 'lo_interior chunked in place', 'lo_interior chunked ping-pong', 'lo_interior block'):
        rows[name] = []

    def hit(name, label):
        rows[name].append(label)

    for label, r in routed_cases():
        dense = label.startswith('dense')
        if dense:
            hit("result in the caller's buffer (dense)" if r.result == 'a' else 'result in the partner buffer (dense: copy back)', label)
        else:
            hit("result in the handle's buffer (resident)" if r.result == 'a' else 'result in the partner buffer (resident: swap)', label)
        for p in r.passes:
            hit(f'{p.form}<{p.param}>', label)
            f = p.form
            if f in ('x_scan', 'x_scan4'):
                hit(f'{f} one segment' if p.nseg == 1 else (f'{f} ragged last segment' if p.last < p.seg else f'{f} full last segment'), label)
            elif f in ('chunked', 'block'):
                unit_name = 'chunk' if f == 'chunked' else 'segment'
                if p.nseg == 1:
                    hit(f'{f} one {unit_name}', label)
                elif p.last < p.seg:
                    hit(f'{f} ragged last {unit_name}', label)
                    if p.last < pm.K_WARM:
                        hit(f'{f} last {unit_name} below the warm-up', label)
                hit(f'{f} axis {p.axis}', label)
                if p.lo_interior:
                    hit('lo_interior block' if f == 'block' else ('lo_interior chunked in place' if p.in_place else 'lo_interior chunked ping-pong'), label)
                if f == 'chunked':
                    hit('chunked in place' if p.in_place else 'chunked ping-pong', label)
                    if p.lanes > 64:
                        hit('chunked two lane blocks', label)
                    if p.param == 128 and p.axis in (0, 1):
                        hit(f'chunked<128> axis {p.axis}', label)
                    if p.N < pm.HORIZON:
                        hit('chunked line shorter than the horizon', label)
                else:
                    assert not p.in_place
                    hit('block one column block' if p.ncb == 1 else 'block two column blocks', label)
                    hit(f'block W%4={p.wmod4}', label)
            else:
                (nsy, nsx), (ly, lx) = p.nseg, p.last
                if nsy == 1:
                    hit('xy one row segment', label)
                    if p.N[0] == pm.XY_ROWS:
                        hit('xy rows at the tile edge', label)
                else:
                    if ly < pm.XY_NET_ROWS:
                        hit('xy ragged last row segment', label)
                    if ly < pm.XY_K:
                        hit('xy last row segment below the warm-up', label)
                if nsx == 1:
                    hit('xy one column segment', label)
                else:
                    if lx < pm.XY_NET_COLS:
                        hit('xy ragged last column segment', label)
                    if lx < pm.XY_K:
                        hit('xy last column segment below the warm-up', label)
                if dense:
                    hit('xy W%8=0 dense', label)
                elif p.wmod4:
                    hit('xy W%4!=0 pitched', label)

    # the knobs
    for value in gp.CHUNK_KNOB_VALUES:
        rows[f'VT_PF_CHUNK={value}'] = [str(s) for s in gp.CHUNK_KNOB_SHAPES
                                        if ('chunked', int(value)) in pm.forms(pm.route_dense(s, env={'VT_PF_CHUNK': value}))]
    plain = [pm.forms(pm.route_dense(s)) for s in gp.KNOB_SHAPES]
    want = {'VT_PF_NO_XY': lambda fs: not any(f == 'xy' for f, _ in fs), 'VT_PF_NO_BLOCK': lambda fs: not any(f == 'block' for f, _ in fs),
            'VT_PF_BLOCK=1': lambda fs: ('block', pm.BLK_VARIANTS[1]) in fs, 'VT_PF_BLOCK=2': lambda fs: ('block', pm.BLK_VARIANTS[2]) in fs}
    for knob in gp.KNOBS:
        (k, v), = knob.items()
        name = k if k.startswith('VT_PF_NO') else f'{k}={v}'
        rows[name] = [str(s) for s, before in zip(gp.KNOB_SHAPES, plain)
                      if pm.forms(pm.route_dense(s, env=knob)) != before and want[name](pm.forms(pm.route_dense(s, env=knob)))]
    # the one-shot pipeline tests of tests/test_gpu_parity.py reach launch_prefilter_axis0_chunks with chunks of 64 and of 128
    for shape, separable in gp.ONESHOT_SHAPES:
        r = pm.route_oneshot(shape, separable)
        assert r is not None, shape
        rows.setdefault(f'one-shot axis-0 chunks of {r.passes[-1].param}', []).append(str(shape))
    rows.setdefault('one-shot axis-0 chunks of 128', [])

    print()
    for name, cases in rows.items():
        print(f'{name:52s} {len(cases):3d}  ' + '; '.join(cases[:3]) + (' ...' if len(cases) > 3 else ''))
    empty = [name for name, cases in rows.items() if not cases]
    assert not empty, empty
    # impulses: every default form has an impulse volume, and every multi-segment one has cuts
    imp = set()
    for shape in gp.IMPULSE_SHAPES:
        r = pm.route_dense(shape)
        imp.update(pm.forms(r))
        assert len(pm.impulse_positions(r, shape)) >= 2, shape
    assert imp >= set(pm.all_default_forms()) - {('x_scan', 1), ('x_scan4', 1)}, set(pm.all_default_forms()) - imp


def test_routes_of_known_shapes():
    """The model on shapes whose route the sources' comments state."""
    assert pm.forms(pm.route_dense((3, 161, 64))) == [('xy', (16, 10)), ('chunked', 64)]                 # D <= 32: axis 0 in place
    assert pm.forms(pm.route_dense((3, 161, 64), aligned16=False)) == [('x_scan', 1), ('chunked', 64), ('chunked', 64)]
    assert pm.forms(pm.route_dense((6, 128, 512), aligned16=False)) == [('x_scan', 8), ('chunked', 64), ('chunked', 64)]
    assert pm.forms(pm.route_resident((512, 512, 512))) == [('xy', (16, 10)), ('block', (16, 18))]
    assert pm.route_resident((512, 512, 512)).result == 'a'
    r = pm.route_dense((300, 260, 64))
    assert pm.forms(r) == [('xy', (16, 10)), ('block', (16, 18))] and r.passes[0].nseg == (3, 1) and r.passes[1].nseg == 2
    assert pm.route_oneshot((40, 20, 20)) is None


# ---------------------------------------------------------------------------------------------------
# the float32 oracle's own distance from float64
# ---------------------------------------------------------------------------------------------------
def test_oracle_distance():
    """r_ref = max|oracle.prefilter - prefilter_f64| / u for every case and both data kinds; the largest is R_REF (rounded up to one
    decimal), the yardstick of the GPU tests."""
    worst, where = 0.0, None
    per_kind = {k: 0.0 for k in gp.KINDS}
    shapes = [s for _, s in gp.CASES] + gp.RESIDENT + [gp.RECYCLED] + gp.CHUNK_KNOB_SHAPES + gp.KNOB_SHAPES
    for shape in dict.fromkeys(shapes):
        for kind in gp.KINDS:
            vol, c64 = gp.make_vol(shape, kind), gp.reference(shape, kind)
            r = float(np.abs(oracle.prefilter(vol) - c64).max()) / pm.unit(c64)
            per_kind[kind] = max(per_kind[kind], r)
            if r > worst:
                worst, where = r, (shape, kind)
    print(f'oracle distance from float64: largest {worst:.3f} u at {where}; per kind {per_kind}; R_REF = {gp.R_REF}')
    assert worst <= gp.R_REF, (worst, where)
    assert gp.R_REF - worst < 0.1, (worst, 'R_REF is the largest measured distance rounded up to one decimal')
