"""Which libvkas entry points the fused heads call, with which arguments: the check that a change to the host code in ops.py
launches exactly what it launched before.  ops.lib is replaced by a proxy that logs every vkas_* call - name, integer and
float arguments, for pointers only whether they are null, for ConvGeom / HeadDesc / Epilogue their fields the same way - then
one scenario runs forward and backward (twice with flat gradient sinks, so that the second step draws on the zero arena) on
seeded inputs.  The log goes to the given file; a SHA-256 of every forward output and of dx (kernels without atomics) follows
it.  Two versions agree when their files are identical.

    python profiles/entry_trace.py SCENARIO OUT.txt [--flat]      SCENARIO: dense | points | wide | nokeep | at_points
    VKAS_POINT_SPARSE_BWD=0 python profiles/entry_trace.py points OUT.txt     (the label-point heads on the dense paths)

One scenario per process: the pack caches and the zero arena start empty."""
import ctypes
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vkit_ocr_model_adaptive_scaling_amd import _lib, ops  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.training import FlatBuffers  # noqa: E402

LOG = []
CIN, P = 96, 24
# the head sets of tests/test_gpu_head_bwd_lowres.py::HEAD_CASES
SETS = {'dense': [((96,), (1,)), ((40, 33), (1, 2)), ((192, 192), (1, 1)), ((48, 40, 33, 33), (1, 2, 4, 4))],
        'points': [((48, 40, 33, 33), (1, 2, 4, 4)), ((96, 64), (1, 4))],
        'wide': [((256,), (2,))], 'nokeep': [((40, 33), (1, 2))], 'at_points': [((48, 40, 33), (1, 2, 4))]}


def show(a, ctype=None):
    if isinstance(a, type(ctypes.byref(ctypes.c_int()))):
        a = a._obj
    if isinstance(a, ctypes.Structure):
        return '{%s}' % ' '.join('%s=%s' % (n, show(getattr(a, n), t)) for n, t in a._fields_)
    if isinstance(a, ctypes.Array):
        return '[%s]' % ' '.join(show(v, a._type_) for v in a)
    if isinstance(a, ctypes.c_void_p) or ctype is ctypes.c_void_p:
        return 'null' if not getattr(a, 'value', a) else 'ptr'
    return 'null' if a is None else repr(a)


class Proxy:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith('vkas_'):
            return fn

        def call(*args):
            types = _lib._SIGS[name][1]
            LOG.append('%s(%s)' % (name, ', '.join(show(a, t) for a, t in zip(args, types))))
            return fn(*args)
        return call


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def digest(tag, t):
    LOG.append('sha256 %s %s' % (tag, hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()))


class _Mark(torch.autograd.Function):
    """identity whose gradient is zero off the label points and says so (what the precise loss does for its point heads)"""

    @staticmethod
    def forward(ctx, y, py, px):
        ctx.pts = (py, px)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        py, px = ctx.pts
        keep = torch.zeros(g.shape[:3], dtype=torch.bool, device=g.device)
        keep[torch.arange(g.shape[0], device=g.device)[:, None], py, px] = True
        return ops.point_sparse((g * keep[..., None]).contiguous(), py, px), None, None


def run(scenario, up, cs, ocs, flat):
    tag = '%s %s c%s' % (scenario, 'UpHeadsFused' if up else 'HeadsFused', '-'.join(map(str, cs)))
    LOG.append('== ' + tag + (' flat' if flat else ''))
    B, h, w = (1, 64, 64) if up else (1, 128, 128)
    H, W = (2 * h, 2 * w) if up else (h, w)
    x = torch.zeros((B, h, w, ops.rup8(CIN)), dtype=torch.bfloat16)
    x[..., :CIN] = rnd((B, h, w, CIN), 1).to(torch.bfloat16)
    params = []
    for i, (c, oc) in enumerate(zip(cs, ocs)):
        params += [rnd((c, CIN, 3, 3), 10 + i, 1.0 / math.sqrt(CIN * 9)), rnd((c,), 20 + i, 0.1), 1 + rnd((c,), 30 + i, 0.1),
                   rnd((c,), 40 + i, 0.1), rnd((oc, c), 50 + i, 1.0 / math.sqrt(c)), rnd((oc,), 60 + i, 0.1)]
    params = [torch.nn.Parameter(p.cuda()) for p in params]
    fb = FlatBuffers([('p%d' % i, p) for i, p in enumerate(params)]) if flat else None
    g = torch.Generator().manual_seed(3)
    py, px = torch.randint(0, H, (B, P), generator=g).cuda(), torch.randint(0, W, (B, P), generator=g).cuda()
    fused = ops.UpHeadsFused if up else ops.HeadsFused
    assert fused.eligible(x, cs, ocs)
    for step in range(2 if flat else 1):
        if flat:
            fb.zero_grad()
        xa = x.cuda().requires_grad_(True)
        if scenario == 'nokeep':
            with torch.no_grad():
                outs = fused.apply(xa, False, False, *params) if up else fused.apply(xa, False, *params)
        elif scenario == 'at_points':  # the first head dense, the others at the label points of the returned upsample
            *outs, xup = ops.UpHeadsFused.apply(xa, True, True, *params[:6])
            outs += ops.HeadsAtPoints.apply(xup, py, px, *params[6:])
        else:
            outs = fused.apply(xa, True, False, *params) if up else fused.apply(xa, True, *params)
        for i, o in enumerate(outs):
            digest('%s step %d out %d' % (tag, step, i), o)
        if scenario == 'nokeep':
            continue
        loss = 0
        for i, (o, oc) in enumerate(zip(outs, ocs)):
            if scenario in ('points', 'at_points') and i > 0:
                o = _Mark.apply(o, py, px)
            loss = loss + (o[..., :oc] * rnd(tuple(o[..., :oc].shape), 70 + i).cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()
        digest('%s step %d dx' % (tag, step), xa.grad)


def main():
    scenario, out = sys.argv[1], sys.argv[2]
    ops.lib = Proxy(ops.lib)
    for cs, ocs in SETS[scenario]:
        for up in ((True,) if scenario == 'at_points' else (False, True)):
            run(scenario, up, cs, ocs, '--flat' in sys.argv)
    with open(out, 'w') as f:
        f.write('\n'.join(LOG) + '\n')
    print(scenario, len(LOG), 'lines ->', out)


if __name__ == '__main__':
    main()
