"""-m gpu: per-tile staging plans shared by the chunk layers of a cubic plane-quad launch on the z-convolved copy (KIND 4).

The first workgroup of a tile that finds no plan with the launch's epoch builds the row-span table and publishes it; later layers
load it.  The plan is integer data, so a launch that shares plans must give the same bits as one with VT_NO_PLANSHARE.  Covered
here: the README sweep at 512^3 in both layer orders (the handle alternates them launch by launch), the in-plane transposed copy
(angles near a quarter turn), two handles of the same shape whose epochs run in step, matrices that change from launch to launch on
one handle (a stale plan accepted would be wrong), a tile count that is not a multiple of the XCD count, and a 1024^3 subset.
"""
import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 3e-6          # filt_bspline against the CPU oracle (the GPU suite's tolerance)


def centre(shape):
    return np.divide(np.subtract(shape, 1), 2, dtype=np.float32)


def rot(ang, shape):
    return vt.utils.transform_matrix(rotation=(0, ang, 0), rotation_units='deg', rotation_order='rzxz', center=centre(shape))


@pytest.fixture(scope='module')
def torch_mod():
    return pytest.importorskip('torch')


def device_volume(torch, shape, seed):
    g = torch.Generator(device='cuda:0')
    g.manual_seed(seed)
    return torch.rand(shape, dtype=torch.float32, device='cuda:0', generator=g)


def shared_vs_unshared(torch, sv, shape, angles, flags=0):
    """Each angle twice, shared and with VT_NO_PLANSHARE; the order of the two flips from angle to angle so that the shared launches
    fall on both layer orders.  Returns the number of launches compared."""
    out = vt.empty(shape, device='gpu:0')
    out2 = vt.empty(shape, device='gpu:0')
    t_out = torch.as_tensor(out, device='cuda:0')
    t_out2 = torch.as_tensor(out2, device='cuda:0')
    try:
        for i, ang in enumerate(angles):
            m = rot(ang, shape)
            runs = ((out, flags), (out2, flags | _native.NO_PLANSHARE))
            for o, f in (runs if i % 2 == 0 else runs[::-1]):
                sv.affine(m, output=o, _flags=f)
                assert sv.info().last_kernel == 8, (ang, f, sv.info().last_kernel)
            sv.synchronize()
            assert torch.equal(t_out, t_out2), (shape, ang, float((t_out - t_out2).abs().max().item()))
    finally:
        out.free()
        out2.free()
    return len(angles)


def test_plan_share_512_sweep_bit_identical(torch_mod):
    torch = torch_mod
    shape = (512, 512, 512)
    vol = device_volume(torch, shape, 512)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    try:
        # the bench's 180 angles (every one: 85..95 degrees run on the in-plane transposed copy)
        assert shared_vs_unshared(torch, sv, shape, [float(a) for a in range(180)]) == 180
    finally:
        sv.close()
        del vol
        torch.cuda.empty_cache()


def test_plan_share_two_handles_interleaved(torch_mod):
    """Two handles of one shape: the same tile count, plan buffers of the same size and epochs that count in step.  Launches
    alternate between the handles with different matrices; a plan read from the other handle's buffer would carry a valid epoch."""
    torch = torch_mod
    shape = (256, 384, 384)
    vols = [device_volume(torch, shape, 7), device_volume(torch, shape, 8)]
    svs = [vt.StaticVolume(v, interpolation='filt_bspline', device='gpu:0') for v in vols]
    outs = [vt.empty(shape, device='gpu:0') for _ in range(2)]
    ref = vt.empty(shape, device='gpu:0')
    t_outs = [torch.as_tensor(o, device='cuda:0') for o in outs]
    t_ref = torch.as_tensor(ref, device='cuda:0')
    try:
        for ang_a, ang_b in ((30.0, 31.0), (31.0, 30.0), (12.0, 57.0), (57.0, 12.0), (89.0, 91.0)):
            svs[0].affine(rot(ang_a, shape), output=outs[0])
            svs[1].affine(rot(ang_b, shape), output=outs[1])
            for k, ang in ((0, ang_a), (1, ang_b)):
                assert svs[k].info().last_kernel == 8
                svs[k].affine(rot(ang, shape), output=ref, _flags=_native.NO_PLANSHARE)
                svs[k].synchronize()
                assert torch.equal(t_outs[k], t_ref), (k, ang)
    finally:
        for o in outs + [ref]:
            o.free()
        for s in svs:
            s.close()
        del vols
        torch.cuda.empty_cache()


def test_plan_share_changing_matrix_same_grid_against_oracle(torch_mod):
    """30 degrees, then 31, 30, 30.5, 150: the same grid shape each time, so every plan slot left by the previous launch would be
    wrong for the next one.  Each result equals the VT_NO_PLANSHARE result and matches the oracle on a block of planes."""
    torch = torch_mod
    shape = (192, 320, 320)
    vol = device_volume(torch, shape, 30)
    host = vol.cpu().numpy()
    pref = oracle.prefilter(host)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    out = vt.empty(shape, device='gpu:0')
    ref = vt.empty(shape, device='gpu:0')
    t_out = torch.as_tensor(out, device='cuda:0')
    t_ref = torch.as_tensor(ref, device='cuda:0')
    d0, nb = 90, 6
    try:
        for ang in (30.0, 31.0, 30.0, 30.5, 150.0, 31.0):
            m = rot(ang, shape)
            sv.affine(m, output=out)
            assert sv.info().last_kernel == 8
            got = out.get_planes(d0, d0 + nb)
            want = oracle.affine_ex(pref, np.asarray(m, np.float64), 'bspline', (nb,) + shape[1:], plane0=0, global_depth=shape[0],
                                    out_plane0=d0)
            err = float(np.abs(got - want).max())
            assert err <= TOL, (ang, err)
            sv.affine(m, output=ref, _flags=_native.NO_PLANSHARE)
            sv.synchronize()
            assert torch.equal(t_out, t_ref), ang
    finally:
        out.free()
        ref.free()
        sv.close()
        del vol
        torch.cuda.empty_cache()


@pytest.mark.parametrize('shape', [(200, 333, 270), (97, 250, 410)])
def test_plan_share_tile_count_not_multiple_of_8(torch_mod, shape):
    """21 x 9 and 16 x 13 tiles per layer: the layers of a tile land on different XCDs, plans are mostly built again -- same bits."""
    torch = torch_mod
    vol = device_volume(torch, shape, 11)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    try:
        shared_vs_unshared(torch, sv, shape, [0.0, 13.0, 30.0, 45.0, 88.0, 90.0, 92.0, 135.0, 179.0], flags=_native.FORCE_TILED)
    finally:
        sv.close()
        del vol
        torch.cuda.empty_cache()


def test_plan_share_1024_subset(torch_mod):
    """BASELINE config #4's size: 2048 tiles per layer, more than the chip keeps resident."""
    torch = torch_mod
    shape = (1024, 1024, 1024)
    vol = device_volume(torch, shape, 1024)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    try:
        shared_vs_unshared(torch, sv, shape, [0.0, 30.0, 89.0, 100.0])
    finally:
        sv.close()
        del vol
        torch.cuda.empty_cache()
        _native.free_cached_memory(0)
