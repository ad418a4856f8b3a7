"""FPN heads at upsampling factors 3 and 4 (the 5x5 smoothing block, fpn.py:41-48,170-174 of the reference) without a GPU:
argument validation of the vkas_upconv5_* entry points and the module / state-dict schema."""
import ctypes

import pytest
import torch

from vkit_ocr_model_adaptive_scaling_amd import _lib


def test_upconv5_entry_points_validate_arguments():
    lib, P = _lib.lib, ctypes.c_void_p
    a = lambda: P(256)  # any aligned non-null address: the checks run before anything is dereferenced or launched
    geom = lambda **kw: _lib.ConvGeom(*[kw.get(k, v) for k, v in dict(B=2, Hin=7, Win=9, Hout=28, Wout=36, Cp=64, ldx=64,
                                                                          KH=5, KW=5, stride=1, pad=2).items()])
    fwd = lambda g, f=4, Np=32, ldo=32, dt=_lib.BF16, x=None: lib.vkas_upconv5_fwd(
        x or a(), ctypes.byref(g), f, a(), Np, None, a(), ldo, dt, None)
    for bad, msg in ((dict(g=geom(), f=5), b'factor'), (dict(g=geom(), f=2), b'factor'),
                     (dict(g=geom(), dt=_lib.F32), b'16-bit'), (dict(g=geom(Hout=27)), b'must be 4 x'),
                     (dict(g=geom(KH=3, KW=3, pad=1)), b'5x5'), (dict(g=geom(Cp=60, ldx=64)), b'Cp=60'),
                     (dict(g=geom(ldx=68)), b'ldx=68'), (dict(g=geom(), Np=30), b'Np=30'),
                     (dict(g=geom(), ldo=24), b'ldo'), (dict(g=geom(), x=P(258)), b'aligned')):
        assert fwd(**bad) == -1, bad
        assert msg in lib.vkas_last_error(), (bad, lib.vkas_last_error())
    assert lib.vkas_upconv5_dgrad(a(), 32, ctypes.byref(geom()), 3, a(), 32, a(), 64, _lib.BF16, None) == -1
    assert b'must be 3 x' in lib.vkas_last_error()
    assert lib.vkas_upconv5_dgrad(a(), 24, ctypes.byref(geom()), 4, a(), 32, a(), 64, _lib.F16, None) == -1
    assert b'lddy' in lib.vkas_last_error()
    assert lib.vkas_upconv5_dgrad(a(), 32, ctypes.byref(geom()), 4, a(), 32, a(), 56, _lib.F16, None) == -1
    assert b'lddx' in lib.vkas_last_error()
    ws = lib.vkas_upconv5_wgrad_ws_bytes(2, 7, 9, 32)
    assert ws == 2 * 8 * 10 * 32 * 2
    assert lib.vkas_upconv5_wgrad(a(), ctypes.byref(geom()), 4, a(), 32, 32, a(), ws - 2, a(), None, _lib.BF16, None) == -1
    assert b'workspace' in lib.vkas_last_error()
    assert lib.vkas_upconv5_wgrad(a(), ctypes.byref(geom()), 4, a(), 32, 32, a(), ws, None, None, _lib.BF16, None) == -1
    assert lib.vkas_upconv5_fold(a(), a(), 20, 60, 24, 64, 5, 0, _lib.BF16, None) == -1 and b'factor' in lib.vkas_last_error()
    assert lib.vkas_upconv5_fold(a(), a(), 20, 60, 16, 64, 4, 0, _lib.BF16, None) == -1 and b'N=20' in lib.vkas_last_error()
    assert lib.vkas_upconv5_fold(a(), a(), 20, 60, 24, 64, 3, 1, _lib.F32, None) == -1 and b'16-bit' in lib.vkas_last_error()
    assert lib.vkas_upconv5_unfold_wgrad(a(), a(), 20, 60, 24, 60, 4, 0, None) == -1 and b'Cp=60' in lib.vkas_last_error()
    # image sizes: 16 phases x 2 x 2 folded taps at f = 4; 3 x 3 per phase slot and 7 x 7 (phase, tap) groups at f = 3
    assert lib.vkas_upconv5_fold_elems(24, 64, 4, 0) == 16 * 24 * 4 * 64
    assert lib.vkas_upconv5_fold_elems(24, 64, 4, 1) == 64 * 64 * 24
    assert lib.vkas_upconv5_fold_elems(24, 64, 3, 0) == 9 * 24 * 9 * 64
    assert lib.vkas_upconv5_fold_elems(24, 64, 3, 1) == 64 * 49 * 24
    assert lib.vkas_upconv5_fold_elems(24, 64, 5, 0) == 0


@pytest.mark.parametrize('factor', [3, 4])
def test_fpn_head_5x5_schema(factor):
    from vkit_ocr_model_adaptive_scaling_amd.model import FpnHead
    from vkit_ocr_model_adaptive_scaling_amd.model.fpn import build_conv5x5_block
    head = FpnHead(100, 4, factor)
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert shapes == {'step1_conv.0.weight': (52, 100, 5, 5), 'step1_conv.0.bias': (52,), 'step1_conv.2.weight': (52,),
                      'step1_conv.2.bias': (52,), 'step2_conv.1.weight': (4, 52), 'step2_conv.1.bias': (4,)}
    assert head.conv5x5 and head.step1_conv[0].padding == (2, 2)
    assert list(build_conv5x5_block(8, 6).state_dict()) == ['0.weight', '0.bias', '2.weight', '2.bias']
    with pytest.raises(NotImplementedError):
        FpnHead(64, 1, upsampling_factor=5)
