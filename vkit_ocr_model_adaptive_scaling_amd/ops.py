"""Autograd ops of the adaptive-scaling hot path, backed by libvkas.so (HIP, gfx950).

Activations travel between ops as NHWC tensors of shape (B, H, W, Cp) in the compute dtype (bf16 or
fp32), Cp = channels rounded up to a multiple of 8 with zero pad channels; a channel slice of a wider
tensor (pixel stride ld > Cp) is accepted everywhere, which is how concatenation stays copy-free on
the consumer side.  Parameters stay fp32 in the reference's own layouts; each op converts what it
needs with the pack kernels.  Every op launches on torch's current HIP stream and allocates through
torch's caching allocator; nothing here falls back to torch math or to the CPU.
"""
import copy
import ctypes
import os
import weakref
from typing import Optional, Sequence, Tuple

import torch
from torch.autograd import Function

from . import _lib
from ._lib import lib, check, ConvGeom, Epilogue

_FLOAT = torch.float32


def rup8(c: int) -> int:
    return (c + 7) // 8 * 8


_DTYPE_CODES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_MFMA_DTYPES = (torch.bfloat16, torch.float16)  # 16-bit storage types with MFMA kernels (fp32 accumulate)


def _dtc(dtype: torch.dtype) -> int:
    try:
        return _DTYPE_CODES[dtype]
    except KeyError:
        raise TypeError(f'unsupported activation dtype {dtype}') from None


def _dt(t: torch.Tensor) -> int:
    return _dtc(t.dtype)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('vkas ops run on the MI355X only (tensor is on %s); there is no CPU fallback' % t.device)


def act_ok(t: torch.Tensor) -> bool:
    if t.dim() != 4 or t.shape[3] % 8 != 0:
        return False
    B, H, W, C = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else C))
    if t.stride(3) != 1 and C > 1:
        return False
    if ld < C or ld % 8 != 0 or t.data_ptr() % 16 != 0:
        return False
    if W > 1 and t.stride(2) != ld:
        return False
    if H > 1 and t.stride(1) != W * ld:
        return False
    if B > 1 and t.stride(0) != H * W * ld:
        return False
    return True


def act_ld(t: torch.Tensor) -> int:
    B, H, W, C = t.shape
    if W > 1:
        return t.stride(2)
    if H > 1:
        return t.stride(1)
    if B > 1:
        return t.stride(0)
    return C


def as_act(t: torch.Tensor) -> torch.Tensor:
    """Return t if it is a valid (possibly channel-sliced) NHWC activation, else a dense copy."""
    return t if act_ok(t) else t.contiguous()


def new_act(B, H, W, Cp, like: torch.Tensor) -> torch.Tensor:
    return torch.empty((B, H, W, Cp), dtype=like.dtype, device=like.device)


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(((nbytes + 3) // 4 + 4,), dtype=_FLOAT, device=device)


def _workspace(what: str, nbytes: int, device) -> torch.Tensor:
    """The byte workspace of an op whose ``*_workspace_bytes`` answered ``nbytes``; a negative answer means the library
    refused the dimensions, and its message is raised."""
    if nbytes < 0:
        check(-1, what)
    return torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=device)


class _ZeroArena:
    """Zero-initialised fp32 scratch for the atomically accumulated weight-gradient images of one training step: the 15
    per-layer ``torch.zeros`` of a backward pass become slices of one buffer that a single fill clears once per step
    (``zero_arena_reset``, called by ``FlatBuffers.zero_grad``).  A slice is handed out once between two resets, so it is
    clean when its kernel starts and may be dirty afterwards; callers ask for arena memory only for buffers that do not
    outlive the step (their contents are unpacked / added into the flat gradient before the optimizer runs).  Without resets
    (no flat optimizer) every request falls back to ``torch.zeros``."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.off = 0      # floats handed out since the last reset
        self.want = 0     # floats asked for since the last reset (sizes the buffer at the next one)
        self.live = False

    def take(self, n: int, device) -> Optional[torch.Tensor]:
        n_al = -(-n // 64) * 64  # 256-byte aligned slices
        self.want += n_al
        if not self.live or self.buf.device != device or self.off + n_al > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n]
        self.off += n_al
        return t

    def reset(self):
        if self.want == 0 and self.off == 0:
            return  # nothing was asked for since the last reset: the buffer (if any) is still clean
        if self.buf is None or self.want > self.buf.numel():
            dev = self.buf.device if self.buf is not None else torch.device('cuda', torch.cuda.current_device())
            self.buf = None
            self.buf = torch.zeros((self.want,), dtype=_FLOAT, device=dev)
        else:
            self.buf.zero_()
        self.off, self.want, self.live = 0, 0, True


_ZERO_ARENA = _ZeroArena()
_NO_ZERO_ARENA = os.environ.get('VKAS_NO_ZERO_ARENA') is not None  # A/B switch


def zero_arena_reset():
    if not _NO_ZERO_ARENA:
        _ZERO_ARENA.reset()


def zeros_f32(n: int, device, step_scratch: bool) -> torch.Tensor:
    """n zeroed floats; step_scratch: the buffer is dead before the step's optimizer update (see _ZeroArena)."""
    if step_scratch and not _NO_ZERO_ARENA:
        t = _ZERO_ARENA.take(n, device)
        if t is not None:
            return t
    return torch.zeros((n,), dtype=_FLOAT, device=device)


# ---------------------------------------------------------------------------------------- raw wrappers
# Packed operands derived from parameters (GEMM weight layouts, padded vectors) are cached between the uses of one
# parameter value: a weight is used by the forward and the backward of both passes of a step, i.e. packed once per
# layout instead of four times.  An entry is valid while the source storage, its autograd version counter and the
# epoch below are unchanged; the fused optimizer writes parameters through the C ABI (no version bump) and bumps the
# epoch instead (training/optimizer.py).
_PACK_CACHE = {}
_PACK_EPOCH = [0]
# Recipes of the cached images that one vkas_pack_many launch can rebuild (conv / depthwise weights of leaf parameters):
# cache key -> (list of _lib.PackDesc, parameters as weak references, their data pointers when the recipe was recorded)
_PACK_PLAN = {}
_PACK_TABLE = [None]  # ((source, image) pointers of all entries, device descriptor table, device block starts, entries, workgroups)


def invalidate_packed_params():
    _PACK_EPOCH[0] += 1
    _PACK_CACHE.clear()
    _PACK_PLAN.clear()


def _plan_pack(k, descs, params):
    _PACK_PLAN[k] = (descs, tuple(weakref.ref(p) for p in params), tuple(p.data_ptr() for p in params))


def _conv_desc(w4: torch.Tensor, out: torch.Tensor, Np: int, Cp: int, mode: int, n_off: int, Nt: int, dtype) -> _lib.PackDesc:
    N, C, KH, KW = w4.shape
    return _lib.PackDesc(w4.data_ptr(), out.data_ptr(), Np * KH * KW * Cp, 0, N, C, KH, KW, Np, Cp, mode, n_off, Nt, _dtc(dtype))


def refresh_packed_params():
    """All parameters were just updated in place (the fused optimizer: training/optimizer.py).  Instead of dropping the
    packed operands and rebuilding them one launch at a time during the next step (~150 launches of a few microseconds),
    rebuild every image with a recorded recipe by ONE vkas_pack_many launch - the parameters and the images keep their
    addresses, so the descriptor table of a model is uploaded once - and drop only the rest."""
    _PACK_EPOCH[0] += 1
    live = {}
    for k, (descs, refs, ptrs) in _PACK_PLAN.items():
        params = [r() for r in refs]
        if k in _PACK_CACHE and all(p is not None and p.data_ptr() == q for p, q in zip(params, ptrs)):
            live[k] = (descs, refs, ptrs)
    for k in list(_PACK_CACHE):
        if k not in live:
            del _PACK_CACHE[k]
    _PACK_PLAN.clear()
    _PACK_PLAN.update(live)
    if not live:
        return
    keys = tuple(live)
    descs = [d for k in keys for d in live[k][0]]
    # the uploaded table is valid while it is byte for byte what would be uploaded now: the same entries pointing at the same
    # buffers in the same layouts (after an invalidate + lazy rebuild the allocator may hand a freed image block to another
    # layout of the same weight: equal pointers, different mode)
    sig = b''.join(bytes(d) for d in descs)
    tab = _PACK_TABLE[0]
    if tab is None or tab[0] != sig:
        arr = (_lib.PackDesc * len(descs))(*descs)
        starts = [0]
        for d in descs:
            starts.append(starts[-1] + lib.vkas_pack_many_blocks(ctypes.byref(d)))
        dev = _PACK_CACHE[keys[0]][2].device
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        tab = (sig, table, torch.tensor(starts, dtype=torch.int32, device=dev), len(descs), starts[-1])
        _PACK_TABLE[0] = tab
    check(lib.vkas_pack_many(_p(tab[1]), _p(tab[2]), tab[3], tab[4], _stream()), 'pack_many')
    for k in keys:
        stamp, refs, out = _PACK_CACHE[k]
        if isinstance(refs, tuple):  # _cached_pack_multi
            params = [r() for r in refs]
            stamp = (tuple(p._version for p in params), _PACK_EPOCH[0], tuple(p.data_ptr() for p in params))
        else:
            src = refs()
            stamp = (src._version, _PACK_EPOCH[0], src.data_ptr())
        _PACK_CACHE[k] = (stamp, refs, out)


def _cached_pack(src: torch.Tensor, key, build):
    # only leaf parameters have a stable identity; anything else (temporaries, concatenated head weights) is rebuilt
    if not (src.is_leaf and src.requires_grad):
        return build()
    k = (id(src), key)
    ent = _PACK_CACHE.get(k)
    stamp = (src._version, _PACK_EPOCH[0], src.data_ptr())
    if ent is not None and ent[0] == stamp and ent[1]() is src:  # the weak reference guards against a recycled id()
        return ent[2]
    out = build()
    _PACK_CACHE[k] = (stamp, weakref.ref(src), out)
    return out


def pack_conv_weight(w: torch.Tensor, Np: int, Cp: int, mode: int, dtype: torch.dtype) -> torch.Tensor:
    def build():
        w4 = w if w.dim() == 4 else w.view(w.shape[0], w.shape[1], 1, 1)
        N, C, KH, KW = w4.shape
        out = torch.empty((Np * KH * KW * Cp,), dtype=dtype, device=w.device)
        check(lib.vkas_pack_conv_weight(_p(w4.contiguous()), _p(out), N, C, KH, KW, Np, Cp, mode,
                                        _dtc(dtype), _stream()), 'pack_conv_weight')
        if w.is_leaf and w.requires_grad and w4.is_contiguous():
            _plan_pack((id(w), key), [_conv_desc(w4, out, Np, Cp, mode, 0, Np, dtype)], [w])
        return out
    key = ('conv', Np, Cp, mode, dtype)
    return _cached_pack(w, key, build)


def _cached_pack_pair(a: torch.Tensor, b: torch.Tensor, key, build):
    """_cached_pack for an operand derived from two parameters (the fused MLP's weight image)."""
    if not (a.is_leaf and a.requires_grad and b.is_leaf and b.requires_grad):
        return build()
    k = (id(a), id(b), key)
    ent = _PACK_CACHE.get(k)
    stamp = (a._version, b._version, _PACK_EPOCH[0], a.data_ptr(), b.data_ptr())
    if ent is not None and ent[0] == stamp and ent[1]() is a and ent[3]() is b:
        return ent[2]
    out = build()
    _PACK_CACHE[k] = (stamp, weakref.ref(a), out, weakref.ref(b))
    return out


_NO_CHAIN = os.environ.get('VKAS_NO_MLP_CHAIN') is not None  # A/B switch: force the two-GEMM layer path


# The kernels exist up to 512 channels.  Up to 256 channels and - round 4, the pair-split kernel with two 256-register waves per
# SIMD (csrc/mlp_chain.hip::mlp_chain_pair_kernel) - for 256 < C <= 384 with C % 16 == 0 (stage 2 of ConvNeXt-T / -S) the
# fused kernels beat the two-GEMM path (stage 2 of config #3: 0.23 + 0.21 ms per layer against 0.29 + 0.29); at 512 channels
# (ConvNeXt-Base) the one-wave-per-SIMD instantiation measured no faster than two GEMMs, so that width stays on the GEMMs.
_CHAIN_MAX_C = int(os.environ.get('VKAS_MLP_CHAIN_MAX_C', '384'))


def _chain_width_ok(C: int) -> bool:
    return C <= min(_CHAIN_MAX_C, 256) or (256 < C <= min(_CHAIN_MAX_C, 384) and C % 16 == 0) or (384 < C <= _CHAIN_MAX_C)


# The pair-split kernel walks the 4C hidden units of its 128 rows serially (48 chunks at C = 384: 85 us however few rows there
# are); below this many rows - the forward-only configurations, M = 6 400 at stage 2 of config #2 - the two ring GEMMs
# (csrc/gemm_mfma.hip::gemm_nt_ring_kernel: 25 + 20 us) are faster.
_NO_CHAIN_LN = os.environ.get('VKAS_NO_CHAIN_LN') is not None  # A/B switch: LayerNorm as its own launch in front of the fused MLP
_CHAIN_PAIR_MIN_ROWS = int(os.environ.get('VKAS_MLP_CHAIN_PAIR_MIN_ROWS', '16384'))


def mlp_chain_eligible(x: torch.Tensor, C: int) -> bool:
    """The fused ConvNeXt MLP kernels (csrc/mlp_chain.hip) cover 16-bit activations with C % 8 == 0, C <= 512."""
    if 256 < C <= 384 and x.shape[0] * x.shape[1] * x.shape[2] < _CHAIN_PAIR_MIN_ROWS:
        return False
    return (not _NO_CHAIN and x.dtype in _MFMA_DTYPES and x.shape[3] == C and _chain_width_ok(C)
            and lib.vkas_mlp_chain_image_elems(C) > 0)


def pack_mlp_chain(w1: torch.Tensor, w2: torch.Tensor, b1: Optional[torch.Tensor], C: int, mode: int,
                   dtype: torch.dtype) -> torch.Tensor:
    """Packed, pre-swizzled weight image of the fused MLP (mode 0 forward incl. b1, 1 backward)."""
    def build():
        img = torch.empty((lib.vkas_mlp_chain_image_elems(C),), dtype=dtype, device=w1.device)
        check(lib.vkas_mlp_chain_pack(_p(w1.contiguous()), _p(w2.contiguous()), _p(b1.contiguous()) if mode == 0 else None, C,
                                      mode, _p(img), _dtc(dtype), _stream()), 'mlp_chain_pack')
        return img
    if mode == 0:  # the forward image also depends on b1: key on (w1, w2) and stamp b1's version into the key
        return _cached_pack_pair(w1, w2, ('chain', C, mode, dtype, b1._version, b1.data_ptr()), build)
    return _cached_pack_pair(w1, w2, ('chain', C, mode, dtype), build)


def pack_dw_weight(w: torch.Tensor, C: int, Cp: int, flip: int) -> torch.Tensor:
    def build():
        out = torch.empty((lib.vkas_dw_weight_elems(Cp),), dtype=_FLOAT, device=w.device)
        check(lib.vkas_pack_dw_weight(_p(w.contiguous()), _p(out), C, Cp, flip, _stream()), 'pack_dw_weight')
        if w.is_leaf and w.requires_grad and w.is_contiguous():
            _plan_pack((id(w), key), [_lib.PackDesc(w.data_ptr(), out.data_ptr(), 105 * Cp, 1, 0, C, 0, 0, 0, Cp, flip, 0, 0, 0)], [w])
        return out
    key = ('dw', C, Cp, flip)
    return _cached_pack(w, key, build)


def pad_vector(v: Optional[torch.Tensor], npad: int) -> Optional[torch.Tensor]:
    if v is None:
        return None
    if v.dim() == 1 and v.numel() == npad and v.is_contiguous():
        return v

    def build():
        flat = v.reshape(-1)
        if flat.numel() == npad and flat.is_contiguous():
            return flat
        out = torch.empty((npad,), dtype=_FLOAT, device=v.device)
        check(lib.vkas_pad_vector(_p(flat.contiguous()), _p(out), flat.numel(), npad, _stream()), 'pad_vector')
        return out
    return _cached_pack(v, ('pad', npad), build)


def _geom(B, Hin, Win, Hout, Wout, Cp, ldx, KH, KW, stride, pad) -> ConvGeom:
    return ConvGeom(B, Hin, Win, Hout, Wout, Cp, ldx, KH, KW, stride, pad)


class LaunchTimer:
    """Optional per-launch HIP-event timing of the implicit-GEMM kernels (bench.py's roofline leg).  Events are
    recorded on torch's current stream, which is the stream the kernels are launched on."""

    def __init__(self):
        self.records = []  # (kind, start_event, end_event, flops, M, N, K, algorithmic bytes)

    def summary(self):
        out = {}
        for kind, s, e, flops, M, N, K, _ in self.records:
            d = out.setdefault(kind, {'launches': 0, 'ms': 0.0, 'flops': 0.0})
            d['launches'] += 1
            d['ms'] += s.elapsed_time(e)
            d['flops'] += flops
        return out


TIMER: Optional[LaunchTimer] = None


def gemm_kernel_name(x, wgrad, geom, Np, lddy=0, head_width=0, flags=0, has_gb=False) -> str:
    """rocprofv3-style short name (profiles/parse_pmc.py) of the kernel this call reaches: the launchers' own plan."""
    if x.dtype not in _MFMA_DTYPES:
        return 'gemm_tn_simple' if wgrad else 'gemm_nt_simple'
    info = _lib.GemmPlanInfo()
    check(lib.vkas_conv_gemm_plan(wgrad, ctypes.byref(geom), Np, lddy, head_width, flags, int(has_gb), None, ctypes.byref(info)),
          'conv_gemm_plan')
    return info.name.decode()


def _timed(kind, x, flops, M, N, K, fn, nbytes=0.0):
    if TIMER is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    TIMER.records.append((kind, s, e, flops, M, N, K, nbytes))
    return r


def conv_gemm(x: torch.Tensor, geom: ConvGeom, Bw: torch.Tensor, Np: int, out: torch.Tensor, mode=_lib.EPI_NONE,
              bias=None, out2=None, aux=None, colscale=None, rowscale=None, rows_per_image=0, patch=0, patch_hw=(0, 0),
              patch_Cp=0, nk=None, head=None):
    if TIMER is not None:
        # algorithmic FLOPs use the logical (unpadded) N and K when the caller knows them
        M = geom.B * geom.Hout * geom.Wout
        N, K = nk if nk is not None else (Np, geom.KH * geom.KW * geom.Cp)
        kind = gemm_kernel_name(x, 0, geom, Np, head_width=max(head.np[i] for i in range(head.n_heads)) if head is not None else 0)
        es = x.element_size()
        nbytes = (geom.B * geom.Hin * geom.Win * geom.Cp + M * Np * ((out is not None) + (out2 is not None) + (aux is not None))) * es
        return _timed(kind, x, 2.0 * M * N * K, M, N, K,
                      lambda: _conv_gemm(x, geom, Bw, Np, out, mode, bias, out2, aux, colscale, rowscale, rows_per_image,
                                         patch, patch_hw, patch_Cp, head), nbytes)
    return _conv_gemm(x, geom, Bw, Np, out, mode, bias, out2, aux, colscale, rowscale, rows_per_image, patch, patch_hw,
                      patch_Cp, head)


def _conv_gemm(x, geom, Bw, Np, out, mode, bias, out2, aux, colscale, rowscale, rows_per_image, patch, patch_hw,
               patch_Cp, head=None):
    epi = Epilogue(mode, _p(bias).value if bias is not None else None, out.data_ptr() if out is not None else None,
                   act_ld(out) if out is not None else 0,
                   out2.data_ptr() if out2 is not None else None, act_ld(out2) if out2 is not None else 0,
                   aux.data_ptr() if aux is not None else None, act_ld(aux) if aux is not None else 0,
                   colscale.data_ptr() if colscale is not None else None,
                   rowscale.data_ptr() if rowscale is not None else None, rows_per_image, patch, patch_hw[0],
                   patch_hw[1], patch_Cp)
    if head is not None:
        epi.head = head
    check(lib.vkas_conv_gemm_fwd(_p(x), ctypes.byref(geom), _p(Bw), Np, ctypes.byref(epi), _dt(x), _stream()),
          'conv_gemm_fwd')
    return out


def grad_sink(param: Optional[torch.Tensor]):
    """(FlatBuffers, index) when ``param`` is a parameter whose .grad is a live view of a flat gradient buffer
    (training.FlatBuffers): the backward ops then add its gradient in place - the weight-gradient GEMM accumulates into the
    view directly when the packed layout equals the reference layout, else the unpack kernel does - and report the
    delivery to the buffer instead of returning a tensor for autograd to add."""
    s = getattr(param, '_vkas_sink', None) if param is not None else None
    return s if s is not None and s[0].grad_view_ok(s[1]) else None


def _accumulate_pieces(pieces):
    """pieces: [(source address, destination address, fp32 count)]; destination += source, 16 pieces per launch"""
    for i in range(0, len(pieces), 16):
        part = pieces[i:i + 16]
        n = len(part)
        src = (ctypes.c_void_p * n)(*[a for a, _, _ in part])
        dst = (ctypes.c_void_p * n)(*[b for _, b, _ in part])
        cnt = (ctypes.c_int * n)(*[c for _, _, c in part])
        check(lib.vkas_accumulate_many(n, src, dst, cnt, _stream()), 'accumulate_many')


def deliver_small_grads(pairs):
    """pairs: [(parameter, gradient tensor or None)].  Gradients of parameters with a flat .grad view (grad_sink) are
    added onto it by ONE vkas_accumulate_many launch and reported as delivered; returns the list to hand to autograd
    (None in those places, the tensor itself otherwise)."""
    out, todo = [], []
    for param, g in pairs:
        s = grad_sink(param) if g is not None else None
        if s is None or g.dtype != _FLOAT or g.numel() != param.numel():
            out.append(g)
        else:
            todo.append((s, param, g.contiguous()))
            out.append(None)
    _accumulate_pieces([(g.data_ptr(), p.grad.data_ptr(), g.numel()) for _, p, g in todo])
    for s, _, _ in todo:
        s[0].grad_delivered(s[1])
    return out


def conv_wgrad(x: torch.Tensor, geom: ConvGeom, dy: torch.Tensor, Np: int, nk=None, with_bias: bool = False,
               x_gelu: bool = False, gw_into: Optional[torch.Tensor] = None, gb_into: Optional[torch.Tensor] = None,
               step_scratch: bool = False, ordered: bool = False):
    """Weight gradient in the packed (Np, K) layout; with_bias also returns the fused bias gradient (Np,): the two
    live in one zero-filled buffer so a single memset covers both.  x_gelu: the input operand is gelu(x).
    gw_into / gb_into: existing fp32 buffers to ACCUMULATE into (the kernels add with atomics) instead of fresh zeros.
    step_scratch: the caller consumes the result before the step ends (zeros_f32).
    ordered: no split over the reduced rows (vkas_conv_gemm_wgrad_ordered) - for a result that is rounded to a 16-bit
    tensor further down, where the last-bit spread of atomically added partial sums would flip roundings from run to run."""
    assert not (ordered and (with_bias or x_gelu or gw_into is not None))
    K = geom.KH * geom.KW * geom.Cp
    n_new = (0 if gw_into is not None else Np * K) + (Np if with_bias and gb_into is None else 0)
    buf = zeros_f32(n_new, x.device, step_scratch) if n_new else None
    gw = gw_into if gw_into is not None else buf[:Np * K]
    gb = None
    if with_bias:
        gb = gb_into if gb_into is not None else buf[n_new - Np:]
    M = geom.B * geom.Hout * geom.Wout

    def run():
        if ordered:
            check(lib.vkas_conv_gemm_wgrad_ordered(_p(x), ctypes.byref(geom), _p(dy), act_ld(dy), Np, _p(gw), _dt(x), _stream()),
                  'conv_gemm_wgrad_ordered')
            return gw
        fn = lib.vkas_conv_gemm_wgrad_gelu if x_gelu else lib.vkas_conv_gemm_wgrad
        check(fn(_p(x), ctypes.byref(geom), _p(dy), act_ld(dy), Np, _p(gw), _p(gb), _dt(x), _stream()), 'conv_gemm_wgrad')
        return (gw, gb) if with_bias else gw
    if TIMER is None:
        return run()
    kind = gemm_kernel_name(x, 1, geom, Np, act_ld(dy), flags=int(x_gelu) + 2 * int(ordered), has_gb=gb is not None)
    N, Kl = nk if nk is not None else (Np, K)
    nbytes = (geom.B * geom.Hin * geom.Win * geom.Cp + M * Np) * x.element_size() + 4.0 * Np * K
    return _timed(kind, x, 2.0 * M * N * Kl, M, N, Kl, run, nbytes)


def unpack_wgrad(gw: torch.Tensor, shape4, Np: int, Cp: int, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed (Np, KH, KW, Cp) weight gradient -> reference layout (N, C, KH, KW); ``into``: add onto that tensor."""
    N, C, KH, KW = shape4
    g = torch.empty((N, C, KH, KW), dtype=_FLOAT, device=gw.device) if into is None else into
    check(lib.vkas_unpack_conv_wgrad(_p(gw), _p(g), N, C, KH, KW, Np, Cp, int(into is not None), _stream()),
          'unpack_conv_wgrad')
    return g


def conv_param_grads(x, geom, dy, Np: int, weight: torch.Tensor, bias: Optional[torch.Tensor], x_gelu: bool = False):
    """Weight and bias gradient of an implicit-GEMM convolution / Linear for autograd: (gw, gb) in the reference layouts,
    with None where the gradient went straight into the parameter's flat .grad view (grad_sink)."""
    w4 = weight if weight.dim() == 4 else weight.view(weight.shape[0], weight.shape[1], 1, 1)
    N, C, KH, KW = w4.shape
    Cp = geom.Cp
    nk = (N, C * KH * KW)
    sw, sb = grad_sink(weight), grad_sink(bias)
    same_layout = KH == 1 and KW == 1 and Np == N and Cp == C  # packed (Np, K) rows are the reference rows
    gw_into = weight.grad.view(-1) if (sw is not None and same_layout) else None
    gb_into = bias.grad if (sb is not None and Np == N) else None
    # with flat gradient sinks nothing of the packed buffer survives the step: the weight image is unpacked into the sink and
    # a bias gradient that is returned to autograd is added onto the sink's view in place (never adopted as .grad)
    scratch = sw is not None and (bias is None or sb is not None)
    r = conv_wgrad(x, geom, dy, Np, nk=nk, with_bias=bias is not None, x_gelu=x_gelu, gw_into=gw_into, gb_into=gb_into,
                   step_scratch=scratch)
    gwp, gbp = r if bias is not None else (r, None)
    if gw_into is not None:
        gw = None
    elif sw is not None:
        unpack_wgrad(gwp, (N, C, KH, KW), Np, Cp, into=weight.grad.view(N, C, KH, KW))
        gw = None
    else:
        gw = unpack_wgrad(gwp, (N, C, KH, KW), Np, Cp).view(weight.shape)
    gb = None
    if bias is not None and gb_into is None:
        # a slice of the step's zero arena must not reach autograd: AccumulateGrad ADOPTS an incoming tensor when the
        # parameter's .grad is None (set_to_none), and the next arena reset would zero the adopted gradient
        gb = gbp[:N].clone() if scratch else gbp[:N]
    if sw is not None:
        sw[0].grad_delivered(sw[1])
    if gb_into is not None:
        sb[0].grad_delivered(sb[1])
    return gw, gb


def colsum(y: torch.Tensor, n_logical: int) -> torch.Tensor:
    B, H, W, Np = y.shape
    M = B * H * W
    out = torch.empty((Np,), dtype=_FLOAT, device=y.device)
    nbytes = lib.vkas_colsum_ws_bytes(M, Np)
    ws = _ws(nbytes, y.device)
    check(lib.vkas_colsum(_p(y), act_ld(y), M, Np, _p(out), 0, _p(ws), nbytes, _dt(y), _stream()), 'colsum')
    return out[:n_logical]


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, C: int, act_gelu: bool,
                  out: Optional[torch.Tensor] = None):
    B, H, W, Cp = x.shape
    M = B * H * W
    y = new_act(B, H, W, Cp, x) if out is None else out
    stats = torch.empty((M, 2), dtype=_FLOAT, device=x.device)
    gamma, beta = pad_vector(gamma, Cp), pad_vector(beta, Cp)
    check(lib.vkas_layernorm_fwd(_p(x), act_ld(x), _p(gamma), _p(beta), _p(y), act_ld(y), _p(stats), M, C, Cp,
                                 int(act_gelu), _dt(x), _stream()), 'layernorm_fwd')
    return y, stats


def layernorm_bwd(x, gamma, beta, stats, dy, C: int, act_gelu: bool, defer: bool = False):
    """defer: leave the per-workgroup partial rows of dgamma | dbeta in the workspace and return (dx, ws, parts) - the caller
    sums them (finalize_many), typically straight into the parameters' gradient views."""
    B, H, W, Cp = x.shape
    M = B * H * W
    dx = new_act(B, H, W, Cp, x)
    nbytes = lib.vkas_layernorm_bwd_ws_bytes(M, Cp)
    ws = _ws(nbytes, x.device)
    gamma, beta = pad_vector(gamma, Cp), pad_vector(beta, Cp)
    if defer:
        check(lib.vkas_layernorm_bwd(_p(x), act_ld(x), _p(gamma), _p(beta), _p(stats), _p(dy), act_ld(dy), _p(dx),
                                     act_ld(dx), None, None, _p(ws), nbytes, M, C, Cp, int(act_gelu), _dt(x),
                                     _stream()), 'layernorm_bwd')
        return dx, ws, lib.vkas_layernorm_bwd_parts(M, Cp)
    dgb = torch.empty((2 * Cp,), dtype=_FLOAT, device=x.device)  # contiguous pair -> one finalize launch
    dg, db = dgb[:Cp], dgb[Cp:]
    check(lib.vkas_layernorm_bwd(_p(x), act_ld(x), _p(gamma), _p(beta), _p(stats), _p(dy), act_ld(dy), _p(dx),
                                 act_ld(dx), _p(dg), _p(db), _p(ws), nbytes, M, C, Cp, int(act_gelu), _dt(x),
                                 _stream()), 'layernorm_bwd')
    return dx, dg[:C], db[:C]


_NO_FINALIZE_MANY = os.environ.get('VKAS_NO_FINALIZE_MANY') is not None  # A/B switch: per-op finalize + accumulate launches


def finalize_many(items):
    """items: [(workspace tensor, first column, partial rows, columns, row pitch, out tensor, accumulate)] -> ONE launch of
    vkas_finalize_many per 8 reductions (second-stage column sums, optionally added onto ``out``)."""
    for i in range(0, len(items), 8):
        part = items[i:i + 8]
        n = len(part)
        src = (ctypes.c_void_p * n)(*[ws.data_ptr() + 4 * col for ws, col, _, _, _, _, _ in part])
        P = (ctypes.c_long * n)(*[p for _, _, p, _, _, _, _ in part])
        nn = (ctypes.c_int * n)(*[c for _, _, _, c, _, _, _ in part])
        ld = (ctypes.c_int * n)(*[l for _, _, _, _, l, _, _ in part])
        dst = (ctypes.c_void_p * n)(*[o.data_ptr() for _, _, _, _, _, o, _ in part])
        acc = (ctypes.c_int * n)(*[int(a) for _, _, _, _, _, _, a in part])
        check(lib.vkas_finalize_many(n, src, P, nn, ld, dst, acc, _stream()), 'finalize_many')


def small_grad_views(params, Cp: int):
    """The parameters' flat gradient views if EVERY one of them can take a Cp-wide column sum directly (FlatBuffers attached,
    no channel padding), else None."""
    if _NO_FINALIZE_MANY:
        return None
    sinks = [grad_sink(p) for p in params]
    if any(s is None for s in sinks):
        return None
    if any(p.numel() != Cp or not p.grad.is_contiguous() or p.grad.dtype != _FLOAT for p in params):
        return None
    return sinks


def resize_fwd(x, size: Tuple[int, int], mode: int, out=None, accumulate=False):
    B, Hin, Win, Cp = x.shape
    Hout, Wout = size
    y = new_act(B, Hout, Wout, Cp, x) if out is None else out
    nbytes = B * Cp * x.element_size() * (Hin * Win + Hout * Wout * (2 if accumulate else 1))
    x2 = mode == 0 and Hout == 2 * Hin and Wout == 2 * Win and Hin > 1 and Win > 1  # the library's exact-x2 kernels
    _timed('resize2x_fwd_kernel' if x2 else 'resize_fwd_kernel', x, 0.0, B * Hout * Wout, Cp, 0,
           lambda: check(lib.vkas_resize_fwd(_p(x), act_ld(x), _p(y), act_ld(y), B, Hin, Win, Hout, Wout, Cp, mode,
                                             int(accumulate), _dt(x), _stream()), 'resize_fwd'), nbytes)
    return y


def resize_bwd(dy, in_size: Tuple[int, int], mode: int):
    B, Hout, Wout, Cp = dy.shape
    Hin, Win = in_size
    dx = new_act(B, Hin, Win, Cp, dy)
    nbytes = B * Cp * dy.element_size() * (Hin * Win + Hout * Wout)
    x2 = mode == 0 and Hout == 2 * Hin and Wout == 2 * Win and Hin > 1 and Win > 1
    wsb = lib.vkas_resize_bwd_ws_bytes(B, Hin, Win, Hout, Wout, Cp)  # > 0: the two-pass (separable) backward of large ratios
    ws = _ws(wsb, dy.device) if wsb else None
    name = 'resize2x_bwd_kernel' if x2 else ('resize_bwd_x+y_kernel' if wsb else 'resize_bwd_kernel')
    _timed(name, dy, 0.0, B * Hout * Wout, Cp, 0,
           lambda: check(lib.vkas_resize_bwd_ws(_p(dy), act_ld(dy), _p(dx), act_ld(dx), _p(ws), wsb, B, Hin, Win, Hout, Wout, Cp,
                                                mode, 0, _dt(dy), _stream()), 'resize_bwd'), nbytes)
    return dx


def copy_channels(x, out, accumulate=False):
    B, H, W, Cp = x.shape
    check(lib.vkas_copy_channels(_p(x), act_ld(x), _p(out), act_ld(out), B * H * W, Cp, int(accumulate), _dt(x),
                                 _stream()), 'copy_channels')
    return out


# ---------------------------------------------------------------------------------------- autograd ops
class ImageToAct(Function):
    """(B,3,H,W) fp32 NCHW raw pixels -> (B,H,W,8) activation (channels 3..7 zero).  The reference's stem is a plain
    nn.Conv2d (convnext.py:106-123), so an input that requires grad receives one: backward converts the stem
    convolution's NHWC input gradient back to (B,3,H,W) fp32.  Training feeds data (train.py:399-403): no gradient is
    computed then (the caller passes need_input_grad=False to the stem convolution as well)."""

    @staticmethod
    def forward(ctx, img: torch.Tensor, dtype: torch.dtype):
        _require_cuda(img)
        if img.dtype != _FLOAT:
            img = img.float()
        img = img.contiguous()
        B, C, H, W = img.shape
        out = torch.empty((B, H, W, 8), dtype=dtype, device=img.device)
        check(lib.vkas_image_nchw_to_nhwc8(_p(img), _p(out), B, C, H, W,
                                           _dtc(dtype), _stream()),
              'image_nchw_to_nhwc8')
        ctx.C = C
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        g = as_act(g)
        B, H, W, Cp = g.shape
        out = torch.empty((B, ctx.C, H, W), dtype=_FLOAT, device=g.device)
        check(lib.vkas_nhwc_to_nchw_f32(_p(g), act_ld(g), _p(out), B, H, W, ctx.C, _dt(g), _stream()), 'nhwc_to_nchw_f32')
        return out, None


def images_to_act(imgs: Sequence[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """Several (B_i,3,H,W) image batches -> ONE (sum B_i, H, W, 8) activation: the layout conversion of each batch writes its
    slice of the result, so the merged pass schedule (model.forward_both) needs no torch.cat of the fp32 images (200 MB copied
    per step at config #3).  Data only: images that require grad take ImageToAct + torch.cat."""
    if any(i.requires_grad for i in imgs) and torch.is_grad_enabled():
        return ImageToAct.apply(torch.cat(list(imgs), 0), dtype)
    _require_cuda(*imgs)
    H, W = imgs[0].shape[2], imgs[0].shape[3]
    out = torch.empty((sum(i.shape[0] for i in imgs), H, W, 8), dtype=dtype, device=imgs[0].device)
    b0 = 0
    for img in imgs:
        if img.dim() != 4 or img.shape[2:] != (H, W):
            raise ValueError('images_to_act: the batches must share their spatial size')
        img = img.detach()
        img = (img if img.dtype == _FLOAT else img.float()).contiguous()
        B, C = img.shape[0], img.shape[1]
        check(lib.vkas_image_nchw_to_nhwc8(_p(img), _p(out[b0:b0 + B]), B, C, H, W, _dtc(dtype), _stream()),
              'image_nchw_to_nhwc8')
        b0 += B
    return out


class Conv(Function):
    """helper.conv1x1 / conv3x3 / pconv2x2 / pconv4x4 (model/helper.py:18-58) as one implicit GEMM.

    x (B,Hin,Win,Cp) activation; weight in the reference layout (N,C,KH,KW) or (N,C); bias (N,) or None.
    Only stride-1 'same' convs (pad = (K-1)/2) and non-overlapping patch convs (stride = K, pad 0) exist on
    this path."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride: int, pad: int, need_input_grad: bool = True):
        _require_cuda(x, weight)
        x = as_act(x)
        w4 = weight if weight.dim() == 4 else weight.view(weight.shape[0], weight.shape[1], 1, 1)
        N, C, KH, KW = w4.shape
        B, Hin, Win, Cp = x.shape
        if Cp != rup8(C):
            raise ValueError(f'Conv: activation has {Cp} (padded) channels, weight expects {C}')
        Hout = (Hin + 2 * pad - KH) // stride + 1
        Wout = (Win + 2 * pad - KW) // stride + 1
        Np = rup8(N)
        Bw = pack_conv_weight(weight, Np, Cp, 0, x.dtype)
        out = new_act(B, Hout, Wout, Np, x)
        geom = _geom(B, Hin, Win, Hout, Wout, Cp, act_ld(x), KH, KW, stride, pad)
        conv_gemm(x, geom, Bw, Np, out, _lib.EPI_NONE, bias=pad_vector(bias, Np), nk=(N, C * KH * KW))
        ctx.save_for_backward(x, weight, bias if bias is not None else torch.empty(0, device=x.device))
        ctx.cfg = (stride, pad, bias is not None, need_input_grad)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        stride, pad, has_bias, need_input_grad = ctx.cfg
        dy = as_act(dy)
        w4 = weight if weight.dim() == 4 else weight.view(weight.shape[0], weight.shape[1], 1, 1)
        N, C, KH, KW = w4.shape
        B, Hin, Win, Cp = x.shape
        _, Hout, Wout, Np = dy.shape
        geom = _geom(B, Hin, Win, Hout, Wout, Cp, act_ld(x), KH, KW, stride, pad)
        gw, gb = conv_param_grads(x, geom, dy, Np, weight, bias if has_bias else None)
        dx = None
        if need_input_grad and ctx.needs_input_grad[0]:
            if stride == 1:
                # dgrad = same-size conv of dy with the 180-degree rotated, in/out swapped kernel
                Bt = pack_conv_weight(weight, Np, Cp, 1, x.dtype)
                dx = new_act(B, Hin, Win, Cp, x)
                g2 = _geom(B, Hout, Wout, Hin, Win, Np, act_ld(dy), KH, KW, 1, KH - 1 - pad)
                conv_gemm(dy, g2, Bt, Cp, dx, _lib.EPI_NONE, nk=(C, N * KH * KW))
            else:
                assert stride == KH == KW and pad == 0
                Bt = pack_conv_weight(weight, Np, Cp, 2, x.dtype)
                full = (Hout * stride == Hin and Wout * stride == Win)
                dx = new_act(B, Hin, Win, Cp, x) if full else torch.zeros_like(x, memory_format=torch.contiguous_format)
                g2 = _geom(B, Hout, Wout, Hout, Wout, Np, act_ld(dy), 1, 1, 1, 0)
                conv_gemm(dy, g2, Bt, KH * KW * Cp, dx, _lib.EPI_PATCH, patch=KH, patch_hw=(Hout, Wout), patch_Cp=Cp,
                          nk=(C * KH * KW, N))
        return dx, gw, gb, None, None, None


def pack_upconv5_weight(w: torch.Tensor, f: int, Np: int, Cp: int, transposed: int, dtype: torch.dtype) -> torch.Tensor:
    """Folded per-phase taps of a (N, C, 5, 5) weight (csrc/upconv5.hip, vkas_upconv5_fold)."""
    def build():
        N, C = w.shape[0], w.shape[1]
        out = torch.empty((lib.vkas_upconv5_fold_elems(Np, Cp, f, transposed),), dtype=dtype, device=w.device)
        check(lib.vkas_upconv5_fold(_p(w.contiguous()), _p(out), N, C, Np, Cp, f, transposed, _dtc(dtype), _stream()),
              'upconv5_fold')
        return out
    return _cached_pack(w, ('upconv5', f, Np, Cp, transposed, dtype), build)


class UpConv5(Function):
    """Nearest x f upsample followed by helper.conv5x5 (pad 2), f in {3, 4}: the smoothing convolution of FpnHead at those
    factors (fpn.py:41-48,170-174), without the upsampled tensor.  Each output phase is a small convolution over x with
    folded taps (csrc/upconv5.hip).  x (B, H, W, Cp) 16-bit activation; weight (N, C, 5, 5); bias (N,) or None; the output
    is (B, f H, f W, rup8(N)).  The backward reads dy densely, so a point-sparse dy (PreciseLoss) needs nothing special."""

    @staticmethod
    def forward(ctx, x, weight, bias, f: int):
        _require_cuda(x, weight)
        x = as_act(x)
        if x.dtype not in _MFMA_DTYPES:
            raise TypeError('UpConv5: 16-bit activations only (fp32 takes upconv5(), the materialised composite)')
        N, C, KH, KW = weight.shape
        B, H, W, Cp = x.shape
        if (KH, KW) != (5, 5) or Cp != rup8(C):
            raise ValueError(f'UpConv5: weight {tuple(weight.shape)} does not fit a {Cp}-channel activation')
        Np = rup8(N)
        Bf = pack_upconv5_weight(weight, f, Np, Cp, 0, x.dtype)
        out = new_act(B, f * H, f * W, Np, x)
        geom = _geom(B, H, W, f * H, f * W, Cp, act_ld(x), 5, 5, 1, 2)
        M = B * f * H * f * W
        kt = (64 if f == 4 else 49) * C  # folded taps of all phases (16 x 2 x 2 at f = 4, 7 x 7 at f = 3) times C
        _timed('upconv5_nt_kernel', x, 2.0 * (M // (f * f)) * N * kt, M, N, kt // (f * f),
               lambda: check(lib.vkas_upconv5_fwd(_p(x), ctypes.byref(geom), f, _p(Bf), Np, _p(pad_vector(bias, Np)), _p(out),
                                                  act_ld(out), _dt(x), _stream()), 'upconv5_fwd'))
        ctx.save_for_backward(x, weight, bias if bias is not None else torch.empty(0, device=x.device))
        ctx.cfg = (f, bias is not None)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        f, has_bias = ctx.cfg
        dy = as_act(dy)
        N, C = weight.shape[0], weight.shape[1]
        B, H, W, Cp = x.shape
        Np = dy.shape[3]
        geom = _geom(B, H, W, f * H, f * W, Cp, act_ld(x), 5, 5, 1, 2)
        dx = None
        if ctx.needs_input_grad[0]:
            Bt = pack_upconv5_weight(weight, f, Np, Cp, 1, x.dtype)
            dx = new_act(B, H, W, Cp, x)
            check(lib.vkas_upconv5_dgrad(_p(dy), act_ld(dy), ctypes.byref(geom), f, _p(Bt), Np, _p(dx), act_ld(dx), _dt(x),
                                         _stream()), 'upconv5_dgrad')
        gw = gb = None
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gm = 9 if f == 3 else 4
            nw = f * f * Np * gm * Cp
            buf = torch.zeros((nw + Np,), dtype=_FLOAT, device=x.device)
            wsb = lib.vkas_upconv5_wgrad_ws_bytes(B, H, W, Np)
            ws = _ws(wsb, x.device)
            check(lib.vkas_upconv5_wgrad(_p(x), ctypes.byref(geom), f, _p(dy), act_ld(dy), Np, _p(ws), wsb, _p(buf[:nw]),
                                         _p(buf[nw:]) if has_bias else None, _dt(x), _stream()), 'upconv5_wgrad')
            gw = torch.empty((N, C, 5, 5), dtype=_FLOAT, device=x.device)
            check(lib.vkas_upconv5_unfold_wgrad(_p(buf[:nw]), _p(gw), N, C, Np, Cp, f, 0, _stream()), 'upconv5_unfold_wgrad')
            gb = buf[nw:nw + N] if has_bias else None
        return dx, gw, gb, None


def upconv5(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], f: int) -> torch.Tensor:
    """conv5x5(nearest_up(x, f)) for f in {3, 4}: the folded kernels (UpConv5) for 16-bit activations.  The fp32 parity
    mode runs the materialised composite instead - Resize (nearest) to (f H, f W), then the generic implicit GEMM with a
    5x5 / pad 2 geometry - which is exact and simple and only meant for checking, not for speed."""
    if f not in (3, 4):
        raise ValueError(f'upconv5: upsampling factor {f} (3 or 4 only)')
    if x.dtype == _FLOAT:
        return Conv.apply(Resize.apply(x, (x.shape[1] * f, x.shape[2] * f), 1), weight, bias, 1, 2)
    return UpConv5.apply(x, weight, bias, f)


class LayerNorm(Function):
    """helper.ln (+ helper.gelu) on an NHWC activation: model/helper.py:96-101."""

    @staticmethod
    def forward(ctx, x, gamma, beta, act_gelu: bool):
        _require_cuda(x, gamma)
        x = as_act(x)
        C = gamma.numel()
        y, stats = layernorm_fwd(x, gamma.contiguous(), beta.contiguous(), C, act_gelu)
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.act_gelu = act_gelu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        sinks = small_grad_views((gamma, beta), x.shape[3])
        if sinks is not None:  # the column sums go straight into the gradient views: one launch instead of finalize + add
            Cp = x.shape[3]
            dx, ws, parts = layernorm_bwd(x, gamma.contiguous(), beta.contiguous(), stats, as_act(dy), gamma.numel(),
                                          ctx.act_gelu, defer=True)
            finalize_many([(ws, 0, parts, Cp, 2 * Cp, gamma.grad, True), (ws, Cp, parts, Cp, 2 * Cp, beta.grad, True)])
            for sk in sinks:
                sk[0].grad_delivered(sk[1])
            return dx, None, None, None
        dx, dg, db = layernorm_bwd(x, gamma.contiguous(), beta.contiguous(), stats, as_act(dy), gamma.numel(),
                                   ctx.act_gelu)
        dg, db = deliver_small_grads([(gamma, dg), (beta, db)])
        return dx, dg, db, None


class MultiLayerNorm(Function):
    """Per-head LayerNorm(+GELU) over channel slices of one wide activation.

    The heads of a pass share their input, so their 3x3 convolutions run as ONE implicit GEMM whose output holds
    every head's channels side by side (slice h = rup8(C_h) channels).  This op normalises each slice separately
    (model/upernext.py:39-45 per head) and, in backward, writes each head's input gradient straight into its slice
    of one gradient buffer, so the shared conv sees a single dy: no per-head dgrad tensors, no gradient adds."""

    @staticmethod
    def forward(ctx, x, act_gelu: bool, *affine):
        _require_cuda(x)
        x = as_act(x)
        gammas, betas = affine[0::2], affine[1::2]
        outs, stats, off = [], [], 0
        for g, b in zip(gammas, betas):
            C = g.numel()
            Cp = rup8(C)
            y, st = layernorm_fwd(x[..., off:off + Cp], g, b, C, act_gelu)
            outs.append(y)
            stats.append(st)
            off += Cp
        if off != x.shape[3]:
            raise ValueError(f'MultiLayerNorm: slices cover {off} of {x.shape[3]} channels')
        ctx.save_for_backward(x, *gammas, *betas, *stats)
        ctx.n = len(gammas)
        ctx.act_gelu = act_gelu
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        saved = ctx.saved_tensors
        x, gammas, betas, stats = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:]
        B, H, W, Ct = x.shape
        dx = new_act(B, H, W, Ct, x)
        grads, off = [], 0
        M = B * H * W
        for g, b, st, dy in zip(gammas, betas, stats, dys):
            C = g.numel()
            Cp = rup8(C)
            dy = as_act(dy)
            xs, dxs = x[..., off:off + Cp], dx[..., off:off + Cp]
            dgb = torch.empty((2 * Cp,), dtype=_FLOAT, device=x.device)
            nbytes = lib.vkas_layernorm_bwd_ws_bytes(M, Cp)
            ws = _ws(nbytes, x.device)
            gp, bp = pad_vector(g, Cp), pad_vector(b, Cp)
            check(lib.vkas_layernorm_bwd(_p(xs), act_ld(xs), _p(gp), _p(bp), _p(st), _p(dy), act_ld(dy), _p(dxs),
                                         act_ld(dxs), _p(dgb[:Cp]), _p(dgb[Cp:]), _p(ws), nbytes, M, C, Cp,
                                         int(ctx.act_gelu), _dt(x), _stream()), 'layernorm_bwd')
            grads.append((dgb[:C], dgb[Cp:Cp + C]))
            off += Cp
        flat = []
        for dg, db in grads:
            flat.extend([dg, db])
        return (dx, None, *flat)


def _cached_pack_multi(params: Sequence[torch.Tensor], key, build):
    """_cached_pack for an operand derived from several parameters (stacked head weights, head affine tables)."""
    if not all(p.is_leaf and p.requires_grad for p in params):
        return build()
    k = (tuple(id(p) for p in params), key)
    ent = _PACK_CACHE.get(k)
    stamp = (tuple(p._version for p in params), _PACK_EPOCH[0], tuple(p.data_ptr() for p in params))
    if ent is not None and ent[0] == stamp and all(r() is p for r, p in zip(ent[1], params)):
        return ent[2]
    out = build()
    _PACK_CACHE[k] = (stamp, tuple(weakref.ref(p) for p in params), out)
    return out


def pack_head_weights(ws: Sequence[torch.Tensor], nps: Sequence[int], Cp: int, mode: int, dtype: torch.dtype) -> torch.Tensor:
    """The heads' 3x3 weights packed side by side (head h = output channels [n0_h, n0_h + np_h)) as one GEMM operand:
    mode 0 forward (Nt, 3, 3, Cp), mode 1 dgrad (Cp, 3, 3, Nt), mode 3 rows (3, Nt, 3, Cp): per kernel row a 1x3 convolution,
    output channel ky * Nt + n (the forward at the neck's height).  Replaces F.pad + torch.cat of the parameters."""
    Nt = sum(nps)

    def build():
        KH, KW = ws[0].shape[2], ws[0].shape[3]
        out = torch.empty((Nt * KH * KW * Cp,), dtype=dtype, device=ws[0].device)
        off = 0
        descs = []
        for w, np_ in zip(ws, nps):
            N, C = w.shape[0], w.shape[1]
            check(lib.vkas_pack_conv_weight_slice(_p(w.contiguous()), _p(out), N, C, KH, KW, np_, Cp, mode, off, Nt,
                                                  _dtc(dtype), _stream()),
                  'pack_conv_weight_slice')
            descs.append(_conv_desc(w, out, np_, Cp, mode, off, Nt, dtype))
            off += np_
        if all(w.is_leaf and w.requires_grad and w.is_contiguous() for w in ws):
            _plan_pack((tuple(id(w) for w in ws), key), descs, list(ws))
        return out
    key = ('heads', tuple(nps), Cp, mode, dtype)
    return _cached_pack_multi(list(ws), key, build)


def pack_head_bias(bs: Sequence[torch.Tensor], cs: Sequence[int], nps: Sequence[int]) -> torch.Tensor:
    """The heads' conv biases side by side, each padded to its np columns (fp32): the bias operand of the fused head GEMM.
    Rebuilt by vkas_pack_many with the other parameter images after an optimizer step (a bias is a 1 x 1 x 1 'weight')."""
    Nt = sum(nps)
    key = ('head_bias', tuple(nps))

    def build():
        t = torch.empty((Nt,), dtype=_FLOAT, device=bs[0].device)
        off, descs = 0, []
        for b, c, np_ in zip(bs, cs, nps):
            src = b.detach().contiguous()
            check(lib.vkas_pad_vector(_p(src), ctypes.c_void_p(t.data_ptr() + 4 * off), c, np_, _stream()), 'pad_vector')
            descs.append(_lib.PackDesc(src.data_ptr(), t.data_ptr(), np_, 0, c, 1, 1, 1, np_, 1, 0, off, Nt, _dtc(_FLOAT)))
            off += np_
        if all(b.is_leaf and b.requires_grad and b.is_contiguous() for b in bs):
            _plan_pack((tuple(id(b) for b in bs), key), descs, list(bs))
        return t
    return _cached_pack_multi(list(bs), key, build)


class _HeadSet:
    """The heads of one fused pass (HeadsFused, UpHeadsFused, HeadsAtPoints), from the flat parameter tuple: per head conv
    weight (c_h, C, 3, 3), conv bias, gamma, beta, wproj (oc_h, c_h), bproj.  Head h owns the columns [offs[h], offs[h + 1])
    of the Nt stacked output channels (np_h = c_h rounded up to a multiple of 8)."""

    def __init__(self, params, Cp: int):
        self.ws, self.bs = params[0::6], params[1::6]
        self.gammas, self.betas, self.wps, self.bps = params[2::6], params[3::6], params[4::6], params[5::6]
        self.n = len(self.ws)
        self.cs = [g.numel() for g in self.gammas]
        self.ocs = [w.shape[0] for w in self.wps]
        self.nps = [rup8(c) for c in self.cs]
        self.offs = [sum(self.nps[:h]) for h in range(self.n + 1)]
        self.Nt, self.C, self.Cp = self.offs[-1], self.ws[0].shape[1], Cp
        assert all(tuple(w.shape) == (c, self.C, 3, 3) for w, c in zip(self.ws, self.cs)) and Cp == rup8(self.C)

    def desc(self, h0: int, h1: int, pw: int, params_ptr, stats_ptr, proj_ptr) -> _lib.HeadDesc:
        """HeadDesc of the heads [h0, h1), their columns counted from offs[h0]"""
        head = _lib.HeadDesc()
        head.n_heads, head.pw = h1 - h0, pw
        for j, h in enumerate(range(h0, h1)):
            head.n0[j], head.np[j], head.c[j], head.oc[j] = self.offs[h] - self.offs[h0], self.nps[h], self.cs[h], self.ocs[h]
        head.params, head.stats, head.proj = params_ptr, stats_ptr, proj_ptr
        return head

    def packed_params(self, pw: int) -> torch.Tensor:
        """(n, 6 pw + 8) fp32: per head gamma | beta | four projection rows | projection bias, each pw wide"""
        def build():
            t = torch.empty((self.n, 6 * pw + 8), dtype=_FLOAT, device=self.ws[0].device)
            for h in range(self.n):
                check(lib.vkas_pack_head_params(_p(self.gammas[h].contiguous()), _p(self.betas[h].contiguous()),
                                                _p(self.wps[h].contiguous()), _p(self.bps[h].contiguous()), self.cs[h],
                                                self.ocs[h], pw, _p(t[h]), _stream()), 'pack_head_params')
            return t
        return _cached_pack_multi([*self.gammas, *self.betas, *self.wps, *self.bps], ('head_params', pw), build)

    def weights(self, mode: int, dtype: torch.dtype, h0: int = 0, h1: Optional[int] = None) -> torch.Tensor:
        return pack_head_weights(self.ws[h0:h1], self.nps[h0:h1], self.Cp, mode, dtype)

    def bias(self) -> torch.Tensor:
        return pack_head_bias(self.bs, self.cs, self.nps)

    def saved(self, small: bool = True):
        """the parameters in the order they go into save_for_backward; small: the affine and projection ones too"""
        return (*self.ws, *self.bs, *((*self.gammas, *self.betas, *self.wps, *self.bps) if small else ()))

    def from_saved(self, tensors) -> '_HeadSet':
        """this head set around the parameters as autograd hands them back (the tail of ctx.saved_tensors from saved() on)"""
        n, hs = self.n, copy.copy(self)
        hs.ws, hs.bs = tensors[:n], tensors[n:2 * n]
        if len(tensors) >= 6 * n:
            hs.gammas, hs.betas, hs.wps, hs.bps = (tensors[i * n:(i + 1) * n] for i in range(2, 6))
        return hs

    def small_grad_views(self, h: int, pw: int, d: torch.Tensor, gbp: torch.Tensor):
        """head h's small gradients - conv bias, gamma, beta, projection weight, projection bias - as views of the packed
        bias gradient gbp (Nt,) and of the head's row d of vkas_head_tail_bwd's dparams"""
        c, oc, o = self.cs[h], self.ocs[h], self.offs[h]
        return [gbp[o:o + c], d[:c], d[pw:pw + c], d[2 * pw:6 * pw].view(4, pw)[:oc, :c], d[6 * pw:6 * pw + oc]]


def _head_bwd_plan(n_heads: int, sp_range, marked, low: bool):
    """The heads' backward paths as ranges (compact, upres, lowres), each (a, b) and possibly empty.  sp_range: None or the
    (s0, s1) of _point_sparse_run, the compact label-point rows; the other heads are the dense run.  It takes the convolution
    kernels at the upsampled resolution (upres); with ``low`` (UpHeadsFused) its heads without a valid label-point mark take the
    matrix products at the neck's resolution (lowres), if they are a prefix or a suffix of it.  A marked dense head (compact path
    off or not applicable) keeps the convolution kernels: its dz is zero off B*P rows, and they sum what the compact path sums."""
    s0, s1 = sp_range if sp_range is not None else (0, 0)
    d0, d1 = (0, n_heads) if sp_range is None else ((0, s0) if s0 > 0 else (s1, n_heads))
    e0, e1 = d0, d0
    if low:
        plain = [h for h in range(d0, d1) if not marked[h]]
        if plain:
            e0, e1 = plain[0], plain[-1] + 1
        if plain != list(range(e0, e1)) or (e0 > d0 and e1 < d1):
            e0, e1 = d0, d0  # not one run at either end: everything on the convolution kernels
    return (s0, s1), ((e1, d1) if e0 == d0 else (d0, e0)), (e0, e1)


def _points_prepare(py: torch.Tensor, px: torch.Tensor, B: int, H: int, W: int):
    """(scratch, pmap, pix, Mp): pixel -> point map (M,) and the points' pixels (Mp = B*P rounded up to 64), views of scratch"""
    P = py.shape[1]
    M, Mp = B * H * W, -(-(B * P) // 64) * 64
    scratch = torch.empty((M + Mp,), dtype=torch.int32, device=py.device)
    pmap, pix = scratch[:M], scratch[M:]
    check(lib.vkas_points_prepare(_p(py), _p(px), B, P, H, W, _p(pmap), _p(pix), Mp, _stream()), 'points_prepare')
    return scratch, pmap, pix, Mp


def _points_gather_patches_up2(x_low: torch.Tensor, pix: torch.Tensor, Mp: int) -> torch.Tensor:
    """the same patches of the x2 bilinear upsample of x_low (B,h,w,Cp), built from x_low itself (bit-identical); pix are
    pixels of the 2h x 2w map"""
    B, h, w, Cp = x_low.shape
    xs = new_act(1, 1, Mp, 9 * Cp, x_low)
    check(lib.vkas_points_gather_patches_up2(_p(x_low), act_ld(x_low), Cp, B, h, w, _p(pix), Mp, _p(xs), _dt(x_low), _stream()),
          'points_gather_patches_up2')
    return xs


def _points_gather_patches(x: torch.Tensor, pix: torch.Tensor, Mp: int) -> torch.Tensor:
    """(1, 1, Mp, 9 Cp): the 3x3 patches of x (B,H,W,Cp) around the pixels pix"""
    B, H, W, Cp = x.shape
    xs = new_act(1, 1, Mp, 9 * Cp, x)
    check(lib.vkas_points_gather_patches(_p(x), act_ld(x), Cp, B, H, W, _p(pix), Mp, _p(xs), _dt(x), _stream()),
          'points_gather_patches')
    return xs


def _head_tail_bwd(heads, h0, h1, pw, hp, z_ptr, ldz, stats_ptr, dp_ptrs, rows, dz, dparams):
    """vkas_head_tail_bwd for heads [h0, h1) whose z columns start at z_ptr: dz (rows, width) and dparams[h0:h1]."""
    PS = 6 * pw + 8
    head = heads.desc(h0, h1, pw, hp.data_ptr() + h0 * PS * 4, stats_ptr, None)
    ptrs = (ctypes.c_void_p * 4)(*dp_ptrs)
    nbytes = lib.vkas_head_tail_bwd_ws_bytes(rows, pw)
    ws_buf = _ws(nbytes, dz.device)
    width = heads.offs[h1] - heads.offs[h0]
    _timed('head_tail_bwd_kernel', dz, 0.0, rows, width, 0,
           lambda: check(lib.vkas_head_tail_bwd(ctypes.c_void_p(z_ptr), ldz, ctypes.byref(head), ptrs, _p(dz), width,
                                                ctypes.c_void_p(dparams.data_ptr() + h0 * PS * 4), _p(ws_buf), nbytes,
                                                rows, _dt(dz), _stream()), 'head_tail_bwd'),
           float(rows) * (2 * width * dz.element_size() + (h1 - h0) * 40))


def _heads_dense_dz(heads, r0, r1, pw, hp, x, z, stats, dps, dparams):
    """dz (B,H,W,width) of the heads [r0, r1) from the dense z, the row statistics and the output gradients dps"""
    B, H, W, _ = x.shape
    M = B * H * W
    dz = new_act(B, H, W, heads.offs[r1] - heads.offs[r0], x)
    _head_tail_bwd(heads, r0, r1, pw, hp, z.data_ptr() + heads.offs[r0] * x.element_size(), heads.Nt,
                   stats.data_ptr() + r0 * M * 8, [dps[h].data_ptr() for h in range(r0, r1)], M, dz, dparams)
    return dz


def _heads_dense_upres(heads, r0, r1, pw, hp, x, z, stats, dps, dparams, gwp, gbp, dx_up):
    """heads [r0, r1) on the convolution kernels at x's resolution: weight / bias gradient into their slices of gwp / gbp;
    dx_up (B,H,W,Cp) or None is written, not added to"""
    B, H, W, Cp = x.shape
    offs, K, C = heads.offs, 9 * Cp, heads.C
    Nd = offs[r1] - offs[r0]
    dz = _heads_dense_dz(heads, r0, r1, pw, hp, x, z, stats, dps, dparams)
    geom = _geom(B, H, W, H, W, Cp, act_ld(x), 3, 3, 1, 1)
    conv_wgrad(x, geom, dz, Nd, nk=(sum(heads.cs[r0:r1]), C * 9), with_bias=True,
               gw_into=gwp[offs[r0] * K:offs[r1] * K], gb_into=gbp[offs[r0]:offs[r1]])
    if dx_up is not None:
        Bt = heads.weights(1, x.dtype, r0, r1)
        g2 = _geom(B, H, W, H, W, Nd, Nd, 3, 3, 1, 1)
        conv_gemm(dz, g2, Bt, Cp, dx_up, _lib.EPI_NONE, nk=(C, sum(heads.cs[r0:r1]) * 9))


def _heads_dense_lowres(heads, r0, r1, pw, hp, x, z, stats, dps, dparams, gwp, gbp, x_low, dx):
    """heads [r0, r1) at x_low's resolution (x is its x2 bilinear upsample): E = U^T of the nine moved copies of dz, then two
    matrix products; dx (B,h,w,Cp) or None, the gradient of x_low itself, is written, not added to"""
    B, H, W, Cp = x.shape
    h_, w_, M = H // 2, W // 2, B * H * W
    offs, K, C, es = heads.offs, 9 * Cp, heads.C, x.element_size()
    Nd = offs[r1] - offs[r0]
    dz = _heads_dense_dz(heads, r0, r1, pw, hp, x, z, stats, dps, dparams)
    E = new_act(B, h_, w_, 9 * Nd, x)
    # conv bias gradient: column sums of dz, as the convolution's weight-gradient kernel delivers them (the column sums
    # of E's centre tap are the same sum, but of values rounded once more) - summed by the E kernel from the centre 2 x 2
    # block every thread loads anyway, so dz is read once
    nbytes = lib.vkas_upconv_adj_colsum_ws_bytes(B, h_, w_, Nd)
    ws_cs = _ws(nbytes, x.device)
    _timed('upconv_adj_colsum_kernel', x, 0.0, M // 4, 9 * Nd, 0,
           lambda: check(lib.vkas_upconv_adj_colsum(_p(dz), act_ld(dz), _p(E), B, h_, w_, Nd, _p(gbp[offs[r0]:offs[r1]]), 1,
                                                    _p(ws_cs), nbytes, _dt(x), _stream()), 'upconv_adj_colsum'),
           float(M) * Nd * es * 3.25)
    del dz
    g1 = _geom(B, h_, w_, h_, w_, Cp, act_ld(x_low), 1, 1, 1, 0)
    gE = conv_wgrad(x_low, g1, E, 9 * Nd, nk=(9 * sum(heads.cs[r0:r1]), C), step_scratch=True)
    check(lib.vkas_upconv_adj_unpack_wgrad(_p(gE), _p(gwp[offs[r0] * K:offs[r1] * K]), Nd, Cp, _stream()),
          'upconv_adj_unpack_wgrad')
    if dx is not None:
        Bt = heads.weights(1, x.dtype, r0, r1)
        g2 = _geom(B, h_, w_, h_, w_, 9 * Nd, 9 * Nd, 1, 1, 1, 0)
        conv_gemm(E, g2, Bt, Cp, dx, _lib.EPI_NONE, nk=(C, sum(heads.cs[r0:r1]) * 9))


def _heads_points_grads(heads, h0, h1, pw, hp, patches, zs, stats_s, dp_ptrs, pix, pmap, n_points, dparams, gw_into, gb_into,
                        step_scratch, dx_into, dx_low=False):
    """Backward of the heads [h0, h1) on compact label-point rows: zs (1,1,Mp,Ns) their z, stats_s their row statistics, dp_ptrs
    their gathered (Mp, 8) output gradients; patches (1,1,Mp,9 Cp) the 3x3 input patches at the points, or a function that
    gathers them (called after the tail backward).  Returns the packed (weight, bias) gradient - accumulated into gw_into /
    gb_into when given, else a fresh buffer (step_scratch: see conv_wgrad); dx_into (B,H,W,Cp) or None receives the input
    gradient, summed per touched pixel on top of what it holds; with dx_low it is (B,h,w,Cp), the gradient of the map the
    points' map is the x2 bilinear upsample of (pix / pmap stay those of the 2h x 2w map)."""
    Mp, Ns, K, C = zs.shape[2], zs.shape[3], 9 * heads.Cp, heads.C
    dzs = new_act(1, 1, Mp, Ns, zs)
    _head_tail_bwd(heads, h0, h1, pw, hp, zs.data_ptr(), Ns, stats_s.data_ptr(), dp_ptrs, Mp, dzs, dparams)
    # weight / bias gradient: (Ns x Mp) . (Mp x 9 Cp) on the gathered 3x3 patches
    xs = patches() if callable(patches) else patches
    g1 = _geom(1, 1, Mp, 1, Mp, K, K, 1, 1, 1, 0)
    gw, gb = conv_wgrad(xs, g1, dzs, Ns, nk=(sum(heads.cs[h0:h1]), C * 9), with_bias=True, gw_into=gw_into, gb_into=gb_into,
                        step_scratch=step_scratch)
    if dx_into is not None:
        # input gradient: D (Mp x 9 Cp, fp32) = dz_s . W with W (Ns x 9 Cp) the rows of the forward weight image -
        # the reduction runs over W's ROWS, i.e. this is the weight-gradient GEMM shape with dz_s^T as the "dy"
        # operand (fp32 result, no 16-bit rounding of the per-tap terms) - then summed per touched pixel onto dx_into
        B, H, W, Cp = dx_into.shape
        Wf = heads.weights(0, zs.dtype)[heads.offs[h0] * K:heads.offs[h1] * K].view(1, 1, Ns, K)
        dzt = dzs.view(Mp, Ns).t().contiguous().view(1, 1, Ns, Mp)
        g3 = _geom(1, 1, Ns, 1, Ns, K, K, 1, 1, 1, 0)
        D = conv_wgrad(Wf, g3, dzt, Mp, nk=(n_points, C * 9), step_scratch=True, ordered=True)
        if dx_low:  # dx_into is the gradient of the map whose x2 upsample the heads read: U^T is applied on the way
            check(lib.vkas_points_scatter3x3_low(_p(D), _p(pix), _p(pmap), Mp, B, H, W, Cp, _p(dx_into), act_ld(dx_into),
                                                 _dt(zs), _stream()), 'points_scatter3x3_low')
        else:
            check(lib.vkas_points_scatter3x3(_p(D), _p(pix), _p(pmap), Mp, B, H, W, Cp, _p(dx_into), act_ld(dx_into), _dt(zs),
                                             _stream()), 'points_scatter3x3')
    return gw, gb


def _deliver_head_weight_grads(heads, gwp, K):
    """per head the 3x3 weight gradient out of the packed (Nt, K) image gwp: unpacked straight into the flat gradient view and
    reported as delivered (None in the returned list), else the unpacked tensor for autograd"""
    gws = []
    for h in range(heads.n):
        sw = grad_sink(heads.ws[h])
        g = unpack_wgrad(gwp[heads.offs[h] * K:heads.offs[h + 1] * K], (heads.cs[h], heads.C, 3, 3), heads.nps[h], heads.Cp,
                         into=heads.ws[h].grad if sw is not None else None)
        if sw is not None:
            sw[0].grad_delivered(sw[1])
        gws.append(None if sw is not None else g)
    return gws


def _deliver_head_small_grads(heads, pw, dparams, gbp, flat_sinks):
    """The heads' small gradients (conv bias, LayerNorm affine, projection), per head in parameter order: with flat .grad views
    they are added in place by vkas_accumulate_many, 16 contiguous pieces per launch (a projection weight row by row), instead
    of one autograd add per parameter (30 launches per step) - None in the returned lists; else the tensor for autograd."""
    outs, pieces, delivered = [], [], []
    for h in range(heads.n):
        c, oc = heads.cs[h], heads.ocs[h]
        out, views = [], heads.small_grad_views(h, pw, dparams[h], gbp)
        for j, (param, g) in enumerate(zip((heads.bs[h], heads.gammas[h], heads.betas[h], heads.wps[h], heads.bps[h]), views)):
            sk = grad_sink(param)
            if sk is None or not param.grad.is_contiguous():
                # handed to autograd: never a view of the step's zero arena (see conv_param_grads)
                out.append(g.clone() if (flat_sinks and j == 0) else g)
                continue
            if g.dim() == 2:  # projection weight: its oc rows lie pw apart
                pieces.extend((g.data_ptr() + 4 * q * pw, param.grad.data_ptr() + 4 * q * c, c) for q in range(oc))
            else:
                pieces.append((g.data_ptr(), param.grad.data_ptr(), g.numel()))
            delivered.append(sk)
            out.append(None)
        outs.append(out)
    _accumulate_pieces(pieces)
    for sk in delivered:
        sk[0].grad_delivered(sk[1])
    return outs


def _heads_eligible(dtype, M: int, channels, out_channels) -> bool:
    return (dtype in _MFMA_DTYPES and M >= 16384 and len(channels) <= 4 and max(rup8(c) for c in channels) <= 512
            and max(out_channels) <= 4)


class HeadsFused(Function):
    """All heads of a pass (model/upernext.py:215-223 or model/fpn.py:165-183, shared upsampled input) as ONE implicit
    GEMM whose epilogue applies each head's LayerNorm -> GELU -> Linear(C -> out_channels) per pixel: forward writes
    only the pre-LN conv output z (needed by backward) and the 1..4 projected channels; the (M, C) activations and
    their gradients never reach HBM.  Backward recomputes them tile-locally (vkas_head_tail_bwd) and feeds one dz into
    the shared conv's dgrad / wgrad.  bf16 / fp16; out_channels <= 4; heads up to 224 channels in the GEMM epilogue, up to
    512 (ConvNeXt-Base / Large) through vkas_head_tail_fwd on z.

    inputs: x (B,H,W,Cp); then per head: conv weight (C_h, Cin, 3, 3), conv bias (C_h), gamma, beta, wproj (oc, C_h),
    bproj (oc).  The weights are packed side by side by the pack kernel (each head padded to a multiple of 8 rows).
    outputs: per head a (B,H,W,8) fp32 activation holding the oc projected channels (columns >= oc are zero)."""

    @staticmethod
    def eligible(x, channels, out_channels) -> bool:
        return _heads_eligible(x.dtype, x.shape[0] * x.shape[1] * x.shape[2], channels, out_channels)

    @staticmethod
    def forward(ctx, x, keep: bool, *params):
        """keep: torch.is_grad_enabled() at the call site (Function.forward itself always runs with grad mode off)."""
        return HeadsFused._forward(ctx, x, None, keep, params)

    @staticmethod
    def _forward(ctx, x, x_low, keep: bool, params):
        """x_low (UpHeadsFused): the neck feature x is the x2 bilinear upsample of; backward then runs at its resolution."""
        _require_cuda(x, params[0])
        x = as_act(x)
        B, H, W, Cp = x.shape
        heads = _HeadSet(params, Cp)
        n_heads, Nt, C = heads.n, heads.Nt, heads.C
        M, wmax, dev = B * H * W, max(heads.nps), x.device
        # up to 224 columns the tail runs in the convolution's epilogue (one 256 x pw tile per head); wider heads
        # (ConvNeXt-Base / Large) take the plain epilogue + vkas_head_tail_fwd over z
        in_epilogue = wmax <= 224
        pw = (128 if wmax <= 128 else (192 if wmax <= 192 else 224)) if in_epilogue else wmax
        hp = heads.packed_params(pw)
        b_cat = heads.bias()
        # z and the row statistics only serve the backward pass: an inference (no-grad) call does not write them
        # (the wide-head path needs z as the tail kernel's input either way)
        z = new_act(B, H, W, Nt, x) if (keep or not in_epilogue) else None
        stats = torch.empty((n_heads, M, 2), dtype=_FLOAT, device=dev) if keep else None
        proj = torch.empty((n_heads, B, H, W, 8), dtype=_FLOAT, device=dev)
        head = heads.desc(0, n_heads, pw, hp.data_ptr(), stats.data_ptr() if keep else None, proj.data_ptr())
        geom = _geom(B, H, W, H, W, Cp, act_ld(x), 3, 3, 1, 1)
        Bw = heads.weights(0, x.dtype)
        if in_epilogue:
            conv_gemm(x, geom, Bw, Nt, z, _lib.EPI_HEAD, bias=b_cat, nk=(sum(heads.cs), C * 9), head=head)
        else:
            conv_gemm(x, geom, Bw, Nt, z, _lib.EPI_NONE, bias=b_cat, nk=(sum(heads.cs), C * 9))
            check(lib.vkas_head_tail_fwd(_p(z), Nt, ctypes.byref(head), M, _dt(x), _stream()), 'head_tail_fwd')
        if keep:
            ctx.save_for_backward(x, z, stats, hp, *heads.saved(), *(() if x_low is None else (x_low,)))
        ctx.heads, ctx.pw, ctx.low = heads, pw, x_low is not None
        return tuple(proj[h] for h in range(n_heads))

    @staticmethod
    def backward(ctx, *dprojs):
        saved = ctx.saved_tensors
        x, z, stats, hp = saved[:4]
        pw, n_heads = ctx.pw, ctx.heads.n
        heads = ctx.heads.from_saved(saved[4:4 + 6 * n_heads])
        # no_up (UpHeadsFused, forward at the neck's height): the upsample was never materialised and slot 0 holds the neck
        # feature.  x then stands for the upsample's shape and type only (no memory behind it) until a path below reads it.
        no_up = getattr(ctx, 'no_up', False)
        if no_up:
            x = x[:, :1, :1, :].expand(x.shape[0], 2 * x.shape[1], 2 * x.shape[2], x.shape[3])
        B, H, W, Cp = x.shape
        Nt, M, K, dev = heads.Nt, B * H * W, 9 * Cp, x.device
        dparams = torch.empty((n_heads, 6 * pw + 8), dtype=_FLOAT, device=dev)
        # packed weight gradient | bias gradient; with flat gradient sinks both are unpacked / added into the sinks below
        flat_sinks = all(grad_sink(p) is not None for p in list(heads.ws) + list(heads.bs))
        gbuf = zeros_f32(Nt * K + Nt, dev, flat_sinks)
        gwp, gbp = gbuf[:Nt * K], gbuf[Nt * K:]
        dps = [torch.zeros((B, H, W, 8), dtype=_FLOAT, device=dev) if dp is None else dp.contiguous().float() for dp in dprojs]
        # heads whose gradient a label-point loss marked (point_sparse) have B*P non-zero rows: they take the compact path
        sp = _point_sparse_run(dprojs, B, H, W) if _POINT_SPARSE else None
        # low: x is the x2 bilinear upsample U of the neck feature x_low (UpHeadsFused).  The dense heads' gradients are then
        # matrix products over the h*w rows of E (csrc/upconv_adj.hip) and dx is the gradient of x_low itself; the label-point
        # heads add their input gradient onto it through U^T point by point (vkas_points_scatter3x3_low); next to a marked
        # dense head, or with _POINTS_LOW_SCATTER off, they scatter into an upsampled-resolution buffer that U^T (resize2x_bwd)
        # adds onto it.
        low, h_, w_ = ctx.low, H // 2, W // 2
        x_low = saved[4 + 6 * n_heads] if low else None
        (s0, s1), (u0, u1), (e0, e1) = _head_bwd_plan(n_heads, sp and sp[:2], [point_mark(d) is not None for d in dprojs], low)
        need_dx = ctx.needs_input_grad[0]
        dx = (new_act(B, h_, w_, Cp, x) if low else new_act(B, H, W, Cp, x)) if need_dx else None
        dx_pts = dx  # where the convolution kernels write and the label-point heads add their input gradient, at x's resolution
        pts_low = low and need_dx and u1 == u0 and sp is not None and _POINTS_LOW_SCATTER
        if pts_low:  # no buffer at x's resolution at all
            dx_pts = None
        elif low and need_dx and u1 == u0:  # low: a buffer of its own; here only the label-point heads add to it, if any
            dx_pts = torch.zeros((B, H, W, Cp), dtype=x.dtype, device=dev) if sp is not None else None
        elif low:
            dx_pts = new_act(B, H, W, Cp, x) if need_dx else None
        elif u1 == u0 and dx is not None:
            dx.zero_()
        if u1 > u0:
            if no_up:  # a marked dense head keeps the convolution kernels at 2h x 2w: they read the upsample itself
                x = resize_fwd(x_low, (H, W), 0)
            _heads_dense_upres(heads, u0, u1, pw, hp, x, z, stats, dps, dparams, gwp, gbp, dx_pts)
        if e1 > e0:
            _heads_dense_lowres(heads, e0, e1, pw, hp, x, z, stats, dps, dparams, gwp, gbp, x_low, dx)
        if sp is not None:
            offs, Ns, py, px = heads.offs, heads.offs[s1] - heads.offs[s0], sp[2], sp[3]
            _, pmap, pix, Mp = _points_prepare(py, px, B, H, W)
            zs = new_act(1, 1, Mp, Ns, x)
            fbuf = torch.empty(((s1 - s0) * Mp * 10,), dtype=_FLOAT, device=dev)
            stats_s, dproj_s = fbuf[:(s1 - s0) * Mp * 2], fbuf[(s1 - s0) * Mp * 2:]
            ptrs = (ctypes.c_void_p * 4)(*[dps[h].data_ptr() for h in range(s0, s1)])
            check(lib.vkas_points_gather_rows(_p(z), Nt, offs[s0], Ns, ctypes.c_void_p(stats.data_ptr() + s0 * M * 8), ptrs,
                                              s1 - s0, M, _p(pix), Mp, _p(zs), _p(stats_s), _p(dproj_s), _dt(x), _stream()),
                  'points_gather_rows')
            if pts_low and e1 == e0:
                dx.zero_()
            patches = (lambda: _points_gather_patches_up2(x_low, pix, Mp)) if no_up else (lambda: _points_gather_patches(x, pix, Mp))
            _heads_points_grads(heads, s0, s1, pw, hp, patches, zs, stats_s,
                                [dproj_s.data_ptr() + j * Mp * 32 for j in range(s1 - s0)], pix, pmap, py.numel(), dparams,
                                gwp[offs[s0] * K:offs[s1] * K], gbp[offs[s0]:offs[s1]], False, dx if pts_low else dx_pts, pts_low)
        if low and dx is not None and not pts_low:
            if dx_pts is not None:  # dx (+)= U^T dx_pts
                _timed('resize2x_bwd_kernel', x, 0.0, M, Cp, 0,
                       lambda: check(lib.vkas_resize_bwd(_p(dx_pts), act_ld(dx_pts), _p(dx), act_ld(dx), B, h_, w_, H, W, Cp, 0,
                                                         int(e1 > e0), _dt(x), _stream()), 'resize_bwd'),
                       B * Cp * x.element_size() * (h_ * w_ * (2 if e1 > e0 else 1) + H * W))
            elif e1 == e0:
                dx.zero_()
        gws = _deliver_head_weight_grads(heads, gwp, K)
        small = _deliver_head_small_grads(heads, pw, dparams, gbp, flat_sinks)
        return (dx, None, *[g for h in range(n_heads) for g in (gws[h], *small[h])])


_HEAD_BWD_UPRES = os.environ.get('VKAS_HEAD_BWD_UPRES') is not None  # A/B switch: head backward at the upsampled resolution
_HEAD_FWD_UPRES = os.environ.get('VKAS_HEAD_FWD_UPRES') is not None  # A/B switch: head forward at the upsampled resolution


class UpHeadsFused(Function):
    """HeadsFused on the x2 bilinear upsample of the neck feature, as ONE autograd node: forward is Resize + HeadsFused
    launch for launch (resize2x_fwd, then the fused head GEMM: bit-identical outputs); backward of the dense heads runs at the
    neck's resolution.  With U the upsample, z = conv3x3(U x) and E_k = U^T (dz moved by tap k) (vkas_upconv_adj, nine maps of
    h x w x N), the input gradient is E (M/4 x 9N) . W (9N x C) - of the neck feature directly - and the weight gradient
    E^T . x: a quarter of the products of the two convolutions at 2h x 2w, neither dx at 2h x 2w nor its U^T pass.  Same sums,
    other order; E is rounded to the storage type once.  VKAS_HEAD_BWD_UPRES=1 keeps Resize + HeadsFused (model side).

    Forward at the neck's height (rows_route; VKAS_HEAD_FWD_UPRES=1 keeps the two launches above): U = Uy (x) Ux and Uy commutes
    with what acts on columns and channels, so X1 = Ux x (B,h,2w,C), T = conv1x3(X1) with 3 Nt output channels (kernel row ky in
    columns ky * Nt + n: half the products of the 3x3 at 2h x 2w, on the row-slab kernel) and z[r] = b + sum_ky (Uy T_ky)[r + ky
    - 1] formed by the pass that runs the head tail (vkas_head_rows_fwd).  U x is not materialised; T (1.5 x z, rounded to the
    storage type once) lives inside the forward only.  z, the statistics and the maps are stored as before: backward unchanged,
    the label-point patches are built from x (vkas_points_gather_patches_up2).

    inputs: x (B,h,w,Cp) 16-bit with h, w > 1, keep, with_up, then the parameters of HeadsFused; outputs as HeadsFused at
    (2h, 2w)."""

    @staticmethod
    def eligible(x, channels, out_channels) -> bool:
        B, h, w, _ = x.shape
        return not _HEAD_BWD_UPRES and h > 1 and w > 1 and _heads_eligible(x.dtype, 4 * B * h * w, channels, out_channels)

    @staticmethod
    def forward(ctx, x, keep: bool, with_up: bool, *params):
        """with_up: also return the upsampled feature (last output) for another consumer - the opt-in label-point forward
        (HeadsAtPoints) reads it; the gradient it receives goes through U^T onto dx in backward."""
        _require_cuda(x, params[0])
        x = as_act(x)
        ctx.with_up = with_up
        if UpHeadsFused.rows_route(x, with_up, params):
            return UpHeadsFused._forward_rows(ctx, x, keep, params)
        up = resize_fwd(x, (2 * x.shape[1], 2 * x.shape[2]), 0)
        outs = HeadsFused._forward(ctx, up, x, keep, params)
        return (*outs, up) if with_up else outs

    @staticmethod
    def rows_route(x, with_up: bool, params) -> bool:
        """16-bit, rows of whole 256-pixel tiles at 2w (the row-slab kernel's condition on X1), heads the row pass holds in a
        lane group (the widths the fused epilogue takes), operands within 32-bit byte offsets, no upsample asked for"""
        B, h, w, Cp = x.shape
        wmax = max(rup8(g.numel()) for g in params[2::6])
        Nt = sum(rup8(g.numel()) for g in params[2::6])
        return (not _HEAD_FWD_UPRES and not with_up and x.dtype in _MFMA_DTYPES and (2 * w) % 256 == 0 and wmax <= 224
                and B * h * 2 * w * Cp * 2 < 0xFFFFFFF0 and 9 * Nt * Cp * 2 < 0xFFFFFFF0)

    @staticmethod
    def _forward_rows(ctx, x, keep: bool, params):
        B, h, w, Cp = x.shape
        H, W = 2 * h, 2 * w
        heads = _HeadSet(params, Cp)
        n_heads, Nt, C = heads.n, heads.Nt, heads.C
        M, wmax, dev, es = B * H * W, max(heads.nps), x.device, x.element_size()
        pw = 128 if wmax <= 128 else (192 if wmax <= 192 else 224)  # as HeadsFused: backward reads the same parameter block
        hp = heads.packed_params(pw)
        b_cat = heads.bias()
        x1 = new_act(B, h, W, Cp, x)
        _timed('resize2x_x_fwd_kernel', x, 0.0, B * h * W, Cp, 0,
               lambda: check(lib.vkas_resize2x_x_fwd(_p(x), act_ld(x), _p(x1), Cp, B, h, w, Cp, _dt(x), _stream()), 'resize2x_x_fwd'),
               3.0 * B * h * w * Cp * es)
        T = new_act(B, h, W, 3 * Nt, x)
        geom = _geom(B, h, W, h, W, Cp, Cp, 1, 3, 1, 1)
        conv_gemm(x1, geom, heads.weights(3, x.dtype), 3 * Nt, T, _lib.EPI_NONE, nk=(3 * sum(heads.cs), C * 3))
        del x1
        z = new_act(B, H, W, Nt, x) if keep else None
        stats = torch.empty((n_heads, M, 2), dtype=_FLOAT, device=dev) if keep else None
        proj = torch.empty((n_heads, B, H, W, 8), dtype=_FLOAT, device=dev)
        head = heads.desc(0, n_heads, pw, hp.data_ptr(), stats.data_ptr() if keep else None, proj.data_ptr())
        # per output element: 3 blends (2 operations each) and their sums, then the tail's ~27 + 6 per projected channel
        _timed('head_rows_fwd_kernel', x, float(M) * sum(heads.cs) * (9 + 21 + 2 * max(heads.ocs)), M, Nt, 0,
               lambda: check(lib.vkas_head_rows_fwd(_p(T), _p(b_cat), ctypes.byref(head), _p(z), B, h, W, Nt, 0, _dt(x), _stream()),
                             'head_rows_fwd'),
               float(M) * (1.5 * Nt * es + (Nt * es if keep else 0) + n_heads * (40 if keep else 32)))
        del T
        if keep:
            ctx.save_for_backward(x, z, stats, hp, *heads.saved(), x)
        ctx.heads, ctx.pw, ctx.low, ctx.no_up = heads, pw, True, True
        return tuple(proj[k] for k in range(n_heads))

    @staticmethod
    def backward(ctx, *gs):
        d_up = None
        if ctx.with_up:
            gs, d_up = gs[:-1], gs[-1]
        out = HeadsFused.backward(ctx, *gs)
        dx = out[0]
        if d_up is not None and dx is not None:  # dx += U^T d_up
            d_up = as_act(d_up)
            B, H, W, Cp = d_up.shape
            _timed('resize2x_bwd_kernel', d_up, 0.0, B * H * W, Cp, 0,
                   lambda: check(lib.vkas_resize_bwd(_p(d_up), act_ld(d_up), _p(dx), act_ld(dx), B, H // 2, W // 2, H, W, Cp, 0, 1,
                                                     _dt(d_up), _stream()), 'resize_bwd'),
                   B * Cp * d_up.element_size() * (H * W // 2 + H * W))
        return (dx, None, None, *out[2:])


class HeadsAtPoints(Function):
    """Opt-in companion of HeadsFused for a TRAINING step: heads whose outputs the loss reads at the label points only
    (the precise pass's offset / angle / distance heads, loss_function/adaptive_scaling.py:167-179,235-262) evaluated AT
    those points only - the 3x3 patches at the (B, P) points are gathered and conv -> LayerNorm -> GELU -> Linear runs on
    B*P rows instead of B*H*W.  The returned (B,H,W,8) maps hold the heads' true outputs at the label points and zeros
    elsewhere, so this is NOT the module API of the reference (forward_precise returns dense maps): it exists for
    TwoPassStep(label_point_forward=True) and is never the default.  Losses and parameter gradients are those of the dense
    evaluation (the loss reads nothing else; tests/test_gpu_model.py::test_label_point_forward_matches_dense).

    inputs: x (B,H,W,Cp), py, px (B,P) int64, then per head the six parameters of HeadsFused."""

    @staticmethod
    def forward(ctx, x, py, px, *params):
        _require_cuda(x, py, px, params[0])
        x = as_act(x)
        if x.dtype not in _MFMA_DTYPES:
            raise ValueError('HeadsAtPoints: 16-bit activations only')
        B, H, W, Cp = x.shape
        heads = _HeadSet(params, Cp)
        n_heads, Ns, C = heads.n, heads.Nt, heads.C
        if n_heads > 4 or max(heads.ocs) > 4 or max(heads.nps) > 512:
            raise ValueError('HeadsAtPoints: at most 4 heads of at most 512 channels and 4 outputs')
        py, px = py.contiguous().long(), px.contiguous().long()
        if py.dim() != 2 or py.shape[0] != B or px.shape != py.shape or py.shape[1] == 0:
            raise ValueError(f'HeadsAtPoints: label points must be (B={B}, P > 0)')
        K, pw, dev = 9 * Cp, max(heads.nps), x.device
        scratch, _, pix, Mp = _points_prepare(py, px, B, H, W)
        xs = _points_gather_patches(x, pix, Mp)
        hp = heads.packed_params(pw)
        b_cat = heads.bias()
        Wf = heads.weights(0, x.dtype)
        zs = new_act(1, 1, Mp, Ns, x)
        g1 = _geom(1, 1, Mp, 1, Mp, K, K, 1, 1, 1, 0)
        conv_gemm(xs, g1, Wf, Ns, zs, _lib.EPI_NONE, bias=b_cat, nk=(sum(heads.cs), C * 9))
        fbuf = torch.empty((n_heads * Mp * 10,), dtype=_FLOAT, device=dev)
        stats_s, proj_s = fbuf[:n_heads * Mp * 2], fbuf[n_heads * Mp * 2:]
        head = heads.desc(0, n_heads, pw, hp.data_ptr(), stats_s.data_ptr(), proj_s.data_ptr())
        check(lib.vkas_head_tail_fwd(_p(zs), Ns, ctypes.byref(head), Mp, _dt(x), _stream()), 'head_tail_fwd')
        proj = torch.zeros((n_heads, B, H, W, 8), dtype=_FLOAT, device=dev)
        for h in range(n_heads):
            check(lib.vkas_points_scatter_vec8(ctypes.c_void_p(proj_s.data_ptr() + h * Mp * 32), _p(pix), Mp, _p(proj[h]),
                                               _stream()), 'points_scatter_vec8')
        ctx.save_for_backward(xs, zs, stats_s, hp, scratch, *heads.saved(small=False))
        ctx.heads, ctx.meta = heads, (pw, (B, H, W, Cp), py.shape[1], Mp, x.dtype)
        return tuple(proj[h] for h in range(n_heads))

    @staticmethod
    def backward(ctx, *dprojs):
        pw, (B, H, W, Cp), P, Mp, dtype = ctx.meta
        saved = ctx.saved_tensors
        xs, zs, stats_s, hp, scratch = saved[:5]
        heads = ctx.heads.from_saved(saved[5:])
        n_heads, M, K, dev = heads.n, B * H * W, 9 * Cp, xs.device
        pmap, pix = scratch[:M], scratch[M:]
        dproj_s = torch.empty((n_heads, Mp, 8), dtype=_FLOAT, device=dev)
        for h in range(n_heads):
            if dprojs[h] is None:
                dproj_s[h].zero_()
            else:
                check(lib.vkas_points_gather_vec8(_p(dprojs[h].contiguous().float()), _p(pix), Mp, _p(dproj_s[h]), _stream()),
                      'points_gather_vec8')
        dparams = torch.empty((n_heads, 6 * pw + 8), dtype=_FLOAT, device=dev)
        dx = torch.zeros((B, H, W, Cp), dtype=dtype, device=dev) if ctx.needs_input_grad[0] else None
        flat_sinks = all(grad_sink(p) is not None for p in list(heads.ws) + list(heads.bs))
        gwp, gbp = _heads_points_grads(heads, 0, n_heads, pw, hp, xs, zs, stats_s, [d.data_ptr() for d in dproj_s], pix, pmap,
                                       B * P, dparams, None, None, flat_sinks, dx)
        gws = _deliver_head_weight_grads(heads, gwp, K)
        # the small gradients go back to autograd as tensors
        grads = [g for h in range(n_heads) for g in (gws[h], *heads.small_grad_views(h, pw, dparams[h], gbp))]
        return (dx, None, None, *grads)


_POINT_SPARSE = os.environ.get('VKAS_POINT_SPARSE_BWD', '1') != '0'
# label-point heads of UpHeadsFused: input gradient straight onto the neck-resolution dx (vkas_points_scatter3x3_low);
# VKAS_POINTS_UPRES_SCATTER=1 keeps the zeroed 2h x 2w buffer + resize2x_bwd (A/B runs, tests)
_POINTS_LOW_SCATTER = os.environ.get('VKAS_POINTS_UPRES_SCATTER', '0') != '1'


def point_sparse(grad: torch.Tensor, py: torch.Tensor, px: torch.Tensor) -> torch.Tensor:
    """Mark ``grad`` - a dense (B, C, H, W) or (B, H, W, C) gradient - as zero everywhere but at the label points (py, px)
    of its images.  The mark is a Python attribute of this very tensor object, stamped with the tensor's version counter:
    autograd hands the same object to the next backward function when the gradient has a single consumer; anything that
    builds a new tensor (an out-of-place sum with another consumer's gradient, a view, a cast) drops the attribute, and
    anything that writes into this tensor - autograd's input buffer accumulates IN PLACE (``old += new``) when it holds the
    last reference, a tensor hook may call ``g.add_()`` - bumps the version, which voids the mark (``point_mark``).  Only
    functions that keep the zero pattern (per-pixel maps) may pass it on (``pass_point_sparse``)."""
    grad._vkas_points = (py, px, grad._version)
    return grad


def point_mark(t: Optional[torch.Tensor]):
    """(py, px) if ``t`` carries a label-point mark that is still valid (nothing wrote into t since it was marked)."""
    m = getattr(t, '_vkas_points', None) if t is not None else None
    if m is None or t._version != m[2]:
        return None
    return m[0], m[1]


def pass_point_sparse(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    pts = point_mark(src)
    if pts is not None:
        point_sparse(dst, pts[0], pts[1])
    return dst


def _point_sparse_run(dprojs, B, H, W):
    """(h0, h1, py, px) when the heads [h0, h1) - a prefix or a suffix of the heads, so that the others stay one contiguous
    run of z columns - all carry the mark of the SAME label points and the compact path pays (points << pixels)."""
    marks = [point_mark(d) for d in dprojs]
    idx = [h for h, m in enumerate(marks) if m is not None]
    if not idx:
        return None
    h0, h1 = idx[0], idx[-1] + 1
    py, px = marks[h0]
    if idx != list(range(h0, h1)) or (h0 > 0 and h1 < len(dprojs)):
        return None
    if any(m[0] is not py or m[1] is not px for m in (marks[h] for h in idx)):
        return None
    if (py.dim() != 2 or py.shape != px.shape or py.shape[0] != B or py.dtype != torch.int64 or px.dtype != torch.int64
            or not py.is_cuda or not py.is_contiguous() or not px.is_contiguous() or py.shape[1] == 0):
        return None
    if py.numel() * 16 > B * H * W:
        return None
    return h0, h1, py, px


class ConvNextLayer(Function):
    """ConvNextBlockLayer.forward (model/convnext.py:29-59): dw7x7 -> LN -> MLP with the layer-scale / stochastic-depth /
    residual epilogue.  bf16 / fp16, C % 8 == 0, C <= 512: the MLP is ONE kernel per direction (csrc/mlp_chain.hip; the 4C-wide
    activation is written once for backward and never read back between the two matrix products); otherwise
    GEMM(C,4C)+GELU -> GEMM(4C,C)+epilogue.  ``rowscale`` is the per-sample keep mask already divided by the keep
    probability (:41-53) or None."""

    @staticmethod
    def forward(ctx, x, dw_w, dw_b, ln_g, ln_b, w1, b1, w2, b2, block_scale, rowscale, keep: bool = True):
        """keep: torch.is_grad_enabled() at the call site (Function.forward itself always runs with grad mode off);
        False = inference, the backward operands h and z are not written."""
        _require_cuda(x, dw_w)
        x = as_act(x)
        B, H, W, Cp = x.shape
        C = dw_w.shape[0]
        M = B * H * W
        dt, st = _dt(x), _stream()
        # depthwise 7x7
        wdw = pack_dw_weight(dw_w, C, Cp, 0)
        y = new_act(B, H, W, Cp, x)
        dwb = pad_vector(dw_b, Cp)
        dw_fwd_name = 'dwconv7x7_mfma_kernel' if x.dtype in _MFMA_DTYPES else 'dwconv7x7_fwd_kernel'  # rocprofv3 names
        _timed(dw_fwd_name, x, 2.0 * 49 * M * C, M, Cp, 49,
               lambda: check(lib.vkas_dwconv7x7_fwd(_p(x), act_ld(x), _p(wdw), _p(dwb), None, 0, _p(y), Cp, B, H, W, Cp, dt,
                                                    st), 'dwconv7x7_fwd'), 2.0 * M * Cp * x.element_size())
        C4 = w1.shape[0]
        C4p = rup8(C4)
        chain = C4 == 4 * C and mlp_chain_eligible(x, C)
        # LayerNorm: inside the fused MLP kernel where that runs (the rows are normalised on their way into the first matrix
        # product; yn / stats are written for backward only), its own launch otherwise
        fuse_ln = chain and not _NO_CHAIN_LN
        if not fuse_ln:
            yn, stats = layernorm_fwd(y, ln_g.contiguous(), ln_b.contiguous(), C, False)
        # MLP
        out = new_act(B, H, W, Cp, x)
        z = new_act(B, H, W, Cp, x)
        cs = pad_vector(block_scale, Cp)
        rs = None if rowscale is None else rowscale.to(_FLOAT).contiguous()
        if chain and fuse_ln:
            h = new_act(B, H, W, C4p, x) if keep else None
            yn = new_act(B, H, W, Cp, x) if keep else None
            stats = torch.empty((M, 2), dtype=_FLOAT, device=x.device) if keep else None
            if not keep:
                z = None
            g = None
            img = pack_mlp_chain(w1, w2, b1, C, 0, x.dtype)
            es = x.element_size()
            lg, lb = pad_vector(ln_g.contiguous(), Cp), pad_vector(ln_b.contiguous(), Cp)
            _timed('mlp_chain_pair_kernel<fwd>' if 256 < C <= 384 else 'mlp_chain_kernel<fwd>', x, 4.0 * M * C * C4, M, C, C4,
                   lambda: check(lib.vkas_mlp_chain_ln_fwd(_p(y), Cp, _p(lg), _p(lb), _p(yn), Cp, _p(stats), _p(img),
                                                           _p(pad_vector(b2, Cp)), _p(x), act_ld(x), _p(cs), _p(rs), H * W,
                                                           _p(h), C4p, _p(z), Cp, _p(out), Cp, M, C, dt, st),
                                 'mlp_chain_ln_fwd'),
                   float(M) * ((5 * Cp + C4p) if keep else 3 * Cp) * es)
            if not keep:
                return out
        elif chain:
            # one kernel: h = yn W1^T + b1 is written once (for backward), gelu(h) goes from the first matrix product
            # into the second in registers, the layer-scale / stochastic-depth / residual epilogue follows
            h = new_act(B, H, W, C4p, x) if keep else None
            if not keep:
                z = None
            g = None
            img = pack_mlp_chain(w1, w2, b1, C, 0, x.dtype)
            es = x.element_size()
            _timed('mlp_chain_pair_kernel<fwd>' if 256 < C <= 384 else 'mlp_chain_kernel<fwd>', x, 4.0 * M * C * C4, M, C, C4,
                   lambda: check(lib.vkas_mlp_chain_fwd(_p(yn), Cp, _p(img), _p(pad_vector(b2, Cp)),
                                                        _p(x), act_ld(x), _p(cs), _p(rs), H * W, _p(h), C4p, _p(z), Cp,
                                                        _p(out), Cp, M, C, dt, st), 'mlp_chain_fwd'),
                   float(M) * ((4 * Cp + C4p) if keep else 3 * Cp) * es)
            if not keep:
                return out
        else:
            h = new_act(B, H, W, C4p, x) if keep else None  # inference: the pre-activation and z are not written
            if not keep:
                z = None
            g = new_act(B, H, W, C4p, x)
            g1 = _geom(B, H, W, H, W, Cp, Cp, 1, 1, 1, 0)
            conv_gemm(yn, g1, pack_conv_weight(w1, C4p, Cp, 0, x.dtype), C4p, h, _lib.EPI_GELU, bias=pad_vector(b1, C4p),
                      out2=g)
            g2 = _geom(B, H, W, H, W, C4p, C4p, 1, 1, 1, 0)
            conv_gemm(g, g2, pack_conv_weight(w2, Cp, C4p, 0, x.dtype), Cp, out, _lib.EPI_SCALE_RES,
                      bias=pad_vector(b2, Cp), out2=z, aux=x, colscale=cs, rowscale=rs, rows_per_image=H * W)
            if not keep:
                return out
        empty = torch.empty(0, device=x.device)
        ctx.save_for_backward(x, y, stats, yn, h, g if g is not None else empty, z, dw_w, ln_g, ln_b, w1, w2, block_scale,
                              rs if rs is not None else empty, b1, dw_b, b2)
        ctx.chain = chain
        ctx.has_rs = rs is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y, stats, yn, h, g, z, dw_w, ln_g, ln_b, w1, w2, block_scale, rs, b1, dw_b, b2 = ctx.saved_tensors
        rs = rs if ctx.has_rs else None
        dout = as_act(dout)
        B, H, W, Cp = x.shape
        C = dw_w.shape[0]
        C4 = w1.shape[0]
        C4p = rup8(C4)
        M = B * H * W
        dt, st, dev = _dt(x), _stream(), x.device
        cs = pad_vector(block_scale, Cp)
        # With flat gradient views on all five small parameters of the layer, the three second-stage column sums of this
        # backward (layer scale / b2, LayerNorm affine, depthwise weight / bias) and their delivery are ONE vkas_finalize_many
        # launch at the end instead of three finalize launches + one accumulate launch: the producers leave their partial rows.
        sinks = small_grad_views((block_scale, b2, ln_g, ln_b, dw_b), Cp)
        # out = x + rs*cs*z  ->  dz, d(block_scale), d(b2)
        dz = new_act(B, H, W, Cp, x)
        nbytes = lib.vkas_scale_res_bwd_ws_bytes(M, Cp)
        ws_sr = _ws(nbytes, dev)
        if sinks is None:
            dsb = torch.empty((2 * Cp,), dtype=_FLOAT, device=dev)
            dscale, db2 = dsb[:Cp], dsb[Cp:]
        else:
            dscale = db2 = None
        check(lib.vkas_scale_res_bwd(_p(dout), act_ld(dout), _p(z), Cp, _p(cs), _p(rs), H * W, _p(dz), Cp, _p(dscale),
                                     _p(db2), _p(ws_sr), nbytes, M, Cp, dt, st), 'scale_res_bwd')
        g2 = _geom(B, H, W, H, W, C4p, C4p, 1, 1, 1, 0)
        g1 = _geom(B, H, W, H, W, Cp, Cp, 1, 1, 1, 0)
        if ctx.chain:
            # dh = (dz W2) * gelu'(h) and dyn = dh W1 in one kernel; gelu(h) for the W2 weight gradient is applied
            # by that GEMM's operand loader
            dh = new_act(B, H, W, C4p, x)
            dyn = new_act(B, H, W, Cp, x)
            imgt = pack_mlp_chain(w1, w2, None, C, 1, x.dtype)
            _timed('mlp_chain_pair_kernel<bwd>' if 256 < C <= 384 else 'mlp_chain_kernel<bwd>', x, 4.0 * M * C * C4, M, C, C4,
                   lambda: check(lib.vkas_mlp_chain_bwd(_p(dz), Cp, _p(imgt), _p(h), C4p, _p(dh), C4p, _p(dyn), Cp, M, C,
                                                        dt, st), 'mlp_chain_bwd'),
                   float(M) * (2 * Cp + 2 * C4p) * x.element_size())
            gw2, _ = conv_param_grads(h, g2, dz, Cp, w2, None, x_gelu=True)
        else:
            # GEMM2: z = g W2^T + b2
            gw2, _ = conv_param_grads(g, g2, dz, Cp, w2, None)
            dh = new_act(B, H, W, C4p, x)
            conv_gemm(dz, g1, pack_conv_weight(w2, Cp, C4p, 1, x.dtype), C4p, dh, _lib.EPI_DGELU, aux=h)
        # GEMM1: h = yn W1^T + b1 (bias gradient fused into the wgrad kernel)
        gw1, db1 = conv_param_grads(yn, g1, dh, C4p, w1, b1)
        if not ctx.chain:
            dyn = new_act(B, H, W, Cp, x)
            conv_gemm(dh, g2, pack_conv_weight(w1, C4p, Cp, 1, x.dtype), Cp, dyn, _lib.EPI_NONE)
        # LayerNorm
        if sinks is None:
            dy, dlg, dlb = layernorm_bwd(y, ln_g.contiguous(), ln_b.contiguous(), stats, dyn, C, False)
        else:
            dy, ws_ln, parts_ln = layernorm_bwd(y, ln_g.contiguous(), ln_b.contiguous(), stats, dyn, C, False, defer=True)
            dlg = dlb = None
        # depthwise: wgrad, then dgrad (+ the residual path) in one kernel
        gdwb = torch.empty((50 * Cp,), dtype=_FLOAT, device=dev)
        gdw, gdb = gdwb[:49 * Cp], gdwb[49 * Cp:]
        nbytes = lib.vkas_dwconv7x7_wgrad_ws_bytes(B, H, W, Cp)
        ws = _ws(nbytes, dev)
        mfma = x.dtype in _MFMA_DTYPES
        _timed('dwconv7x7_wgrad_mfma_kernel' if mfma else 'dwconv7x7_wgrad_kernel', x, 2.0 * 49 * M * C, M, Cp, 49,
               lambda: check(lib.vkas_dwconv7x7_wgrad(_p(x), act_ld(x), _p(dy), Cp, _p(gdw) if sinks is None else None,
                                                      _p(gdb) if sinks is None else None, _p(ws), nbytes, B, H, W,
                                                      Cp, dt, st), 'dwconv7x7_wgrad'), 2.0 * M * Cp * x.element_size())
        if sinks is not None:
            p_sr = lib.vkas_scale_res_bwd_parts(M, Cp)
            p_dw = lib.vkas_dwconv7x7_wgrad_parts(B, H, W, Cp, dt)
            finalize_many([(ws_sr, 0, p_sr, Cp, 2 * Cp, block_scale.grad, True), (ws_sr, Cp, p_sr, Cp, 2 * Cp, b2.grad, True),
                           (ws_ln, 0, parts_ln, Cp, 2 * Cp, ln_g.grad, True), (ws_ln, Cp, parts_ln, Cp, 2 * Cp, ln_b.grad, True),
                           (ws, 0, p_dw, 49 * Cp, 50 * Cp, gdw, False), (ws, 49 * Cp, p_dw, Cp, 50 * Cp, dw_b.grad, True)])
            for sk in sinks:
                sk[0].grad_delivered(sk[1])
        sdw = grad_sink(dw_w)
        if sdw is not None:  # unpack straight onto the flat gradient view
            check(lib.vkas_unpack_dw_wgrad(_p(gdw), _p(dw_w.grad), C, Cp, 1, st), 'unpack_dw_wgrad')
            sdw[0].grad_delivered(sdw[1])
            gdw_ref = None
        else:
            gdw_ref = torch.empty((C, 1, 7, 7), dtype=_FLOAT, device=dev)
            check(lib.vkas_unpack_dw_wgrad(_p(gdw), _p(gdw_ref), C, Cp, 0, st), 'unpack_dw_wgrad')
        dx = None
        if ctx.needs_input_grad[0]:
            wflip = pack_dw_weight(dw_w, C, Cp, 1)
            dx = new_act(B, H, W, Cp, x)
            _timed('dwconv7x7_mfma_kernel' if mfma else 'dwconv7x7_fwd_kernel', x, 2.0 * 49 * M * C, M, Cp, 49,
                   lambda: check(lib.vkas_dwconv7x7_fwd(_p(dy), Cp, _p(wflip), None, _p(dout), act_ld(dout), _p(dx), Cp, B, H,
                                                        W, Cp, dt, st), 'dwconv7x7_dgrad'), 3.0 * M * Cp * x.element_size())
        if sinks is not None:
            return (dx, gdw_ref, None, None, None, gw1, db1, gw2, None, None, None, None)
        gdb_, dlg, dlb, db2_, dsc = deliver_small_grads([(dw_b, gdb[:C]), (ln_g, dlg), (ln_b, dlb), (b2, db2[:C]),
                                                         (block_scale, dscale[:C].view(block_scale.shape))])
        return (dx, gdw_ref, gdb_, dlg, dlb, gw1, db1, gw2, db2_, dsc, None, None)


class Resize(Function):
    """F.interpolate to an explicit size; mode 0 bilinear/align_corners=False (model/upernext.py:79,191-195,237-244),
    mode 1 nearest (model/fpn.py:138-142,197-204)."""

    @staticmethod
    def forward(ctx, x, size, mode: int):
        _require_cuda(x)
        x = as_act(x)
        ctx.in_size = (x.shape[1], x.shape[2])
        ctx.mode = mode
        return resize_fwd(x, tuple(size), mode)

    @staticmethod
    def backward(ctx, dy):
        return resize_bwd(as_act(dy), ctx.in_size, ctx.mode), None, None


class ResizeAdd(Function):
    """dst += F.interpolate(src, dst.shape) in place (model/upernext.py:174-182, model/fpn.py:121-129).  Legal for
    the same reason as in the reference: the producer of dst saved its input, not its output."""

    @staticmethod
    def forward(ctx, dst, src, mode: int):
        _require_cuda(dst, src)
        if not act_ok(dst):
            raise ValueError('ResizeAdd: dst must be a valid NHWC activation')
        src = as_act(src)
        ctx.in_size = (src.shape[1], src.shape[2])
        ctx.mode = mode
        resize_fwd(src, (dst.shape[1], dst.shape[2]), mode, out=dst, accumulate=True)
        ctx.mark_dirty(dst)
        return dst

    @staticmethod
    def backward(ctx, dy):
        dy = as_act(dy)
        return dy, resize_bwd(dy, ctx.in_size, ctx.mode), None


class AdaptiveAvgPool(Function):
    """nn.AdaptiveAvgPool2d(s) (model/upernext.py:62)."""

    @staticmethod
    def forward(ctx, x, s: int):
        _require_cuda(x)
        x = as_act(x)
        B, H, W, Cp = x.shape
        y = new_act(B, s, s, Cp, x)
        check(lib.vkas_adaptive_avgpool_fwd(_p(x), act_ld(x), _p(y), Cp, B, H, W, s, Cp, _dt(x), _stream()),
              'adaptive_avgpool_fwd')
        ctx.cfg = (H, W, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        H, W, s = ctx.cfg
        dy = as_act(dy)
        B, _, _, Cp = dy.shape
        dx = new_act(B, H, W, Cp, dy)
        check(lib.vkas_adaptive_avgpool_bwd(_p(dy), act_ld(dy), _p(dx), Cp, B, H, W, s, Cp, 0, _dt(dy), _stream()),
              'adaptive_avgpool_bwd')
        return dx, None


class AdaptiveAvgPools(Function):
    """[nn.AdaptiveAvgPool2d(s)(x) for s in scales] (the PPM's pooled branches, model/upernext.py:58-66) as one autograd node:
    backward adds the branches' gradients inside the pooling kernels (accumulate flag) instead of leaving len(scales) - 1 adds
    of full-size tensors to the autograd engine."""

    @staticmethod
    def forward(ctx, x, *scales: int):
        _require_cuda(x)
        x = as_act(x)
        B, H, W, Cp = x.shape
        ys = []
        for s in scales:
            y = new_act(B, s, s, Cp, x)
            check(lib.vkas_adaptive_avgpool_fwd(_p(x), act_ld(x), _p(y), Cp, B, H, W, s, Cp, _dt(x), _stream()),
                  'adaptive_avgpool_fwd')
            ys.append(y)
        ctx.cfg = (B, H, W, Cp, tuple(scales), x.dtype, x.device)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        B, H, W, Cp, scales, dtype, dev = ctx.cfg
        dx = torch.empty((B, H, W, Cp), dtype=dtype, device=dev)
        first = True
        for s, dy in zip(scales, dys):
            if dy is None:
                continue
            dy = as_act(dy)
            check(lib.vkas_adaptive_avgpool_bwd(_p(dy), act_ld(dy), _p(dx), Cp, B, H, W, s, Cp, 0 if first else 1, _dt(dy),
                                                _stream()), 'adaptive_avgpool_bwd')
            first = False
        if first:
            dx.zero_()
        return (dx,) + (None,) * len(scales)


class Cat(Function):
    """torch.cat along channels (model/upernext.py:82,197, model/fpn.py:144): each part is written into its channel
    slice of one NHWC buffer; backward hands out slices (views) of the incoming gradient."""

    @staticmethod
    def forward(ctx, *parts):
        _require_cuda(*parts)
        parts = [as_act(p) for p in parts]
        B, H, W, _ = parts[0].shape
        widths = [p.shape[3] for p in parts]
        out = new_act(B, H, W, sum(widths), parts[0])
        off = 0
        for p, w in zip(parts, widths):
            copy_channels(p, out[..., off:off + w])
            off += w
        ctx.widths = widths
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = as_act(dy)
        outs, off = [], 0
        for w in ctx.widths:
            outs.append(dy[..., off:off + w])
            off += w
        return tuple(outs)


def copy_channel_range(x, c_src: int, out, c_dst: int, C: int, zero_tail: int = 0):
    """out[..., c_dst : c_dst + C] = x[..., c_src : c_src + C] (then ``zero_tail`` zero channels): channel offsets at
    element granularity, for concatenations whose parts are not multiples of 8 channels wide."""
    B, H, W, _ = x.shape
    check(lib.vkas_copy_channel_range(_p(x), act_ld(x), c_src, _p(out), act_ld(out), c_dst, B * H * W, C, zero_tail, _dt(x),
                                      _stream()), 'copy_channel_range')
    return out


class ResizeCat(Function):
    """torch.cat([first] + [F.interpolate(p, first's size) for p in others], channels) (model/upernext.py:184-197): the
    resize kernels write straight into their channel slice of the concatenated buffer, so only ``first`` is copied; backward
    reads each slice of the incoming gradient in place.

    ``widths``: the parts' LOGICAL channel counts, or None when every part is as wide as its activation.  The reference
    only asks for ``out_channels % len(levels) == 0`` (upernext.py:144, fpn.py:75) and its own test builds
    ``FpnNeck(..., out_channels=400)`` = 4 x 100 channels (tests/test_fpn.py:16-28): torch.cat puts the parts side by side
    WITHOUT pad channels, so part i starts at channel 100 i - not a 16-byte boundary.  Such a concatenation takes the
    compact path: every part is resized into a buffer of its own and moved to its element-granular channel offset by
    vkas_copy_channel_range; backward cuts the gradient's slices out into zero-padded buffers the same way."""

    @staticmethod
    def forward(ctx, mode: int, widths, first, *others):
        _require_cuda(first, *others)
        first = as_act(first)
        others = [as_act(p) for p in others]
        B, H, W, w0 = first.shape
        padded = [w0] + [p.shape[3] for p in others]
        widths = padded if widths is None else [int(w) for w in widths]
        if len(widths) != len(padded) or any(rup8(w) != pw for w, pw in zip(widths, padded)):
            raise ValueError(f'ResizeCat: logical widths {widths} do not match the activations\' channels {padded}')
        ctx.cfg = (mode, widths, [(p.shape[1], p.shape[2]) for p in others])
        if all(w % 8 == 0 for w in widths):
            out = new_act(B, H, W, sum(widths), first)
            copy_channels(first, out[..., :w0])
            off = w0
            for p in others:
                resize_fwd(p, (H, W), mode, out=out[..., off:off + p.shape[3]])
                off += p.shape[3]
            return out
        total = sum(widths)
        out = new_act(B, H, W, rup8(total), first)
        off = 0
        for i, (p, w) in enumerate(zip([first] + others, widths)):
            r = p if i == 0 else resize_fwd(p, (H, W), mode)
            last = i == len(widths) - 1
            copy_channel_range(r, 0, out, off, w, (rup8(total) - total) if last else 0)
            off += w
        return out

    @staticmethod
    def backward(ctx, dy):
        mode, widths, in_sizes = ctx.cfg
        dy = as_act(dy)
        if all(w % 8 == 0 for w in widths):
            grads = [dy[..., :widths[0]]]
            off = widths[0]
            for w, size in zip(widths[1:], in_sizes):
                grads.append(resize_bwd(dy[..., off:off + w], size, mode))
                off += w
            return (None, None, *grads)
        B, H, W, _ = dy.shape
        grads, off = [], 0
        for i, w in enumerate(widths):
            g = new_act(B, H, W, rup8(w), dy)
            copy_channel_range(dy, off, g, 0, w, rup8(w) - w)  # pad channels of an activation gradient are zero
            grads.append(g if i == 0 else resize_bwd(g, in_sizes[i - 1], mode))
            off += w
        return (None, None, *grads)


# limits of csrc/ppm.hip (VKAS_PPM_* of include/vkas.h; its entry points check them again)
PPM_MAX_BRANCHES, PPM_MAX_SCALE, PPM_MAX_CELLS, PPM_MAX_C, PPM_MAX_CB = 4, 16, 256, 2048, 512


def ppm_fused_eligible(dtype: torch.dtype, C: int, Cb: int, scales: Sequence[int]) -> bool:
    """Whether PpmBranchesCat runs a pyramid-pooling block of C input and Cb branch channels at these scales: 16-bit
    storage, channel counts that are their own padded widths, and the kernels' limits.  The map size is free."""
    scales = tuple(scales)
    return (dtype in _MFMA_DTYPES and C % 8 == 0 and Cb % 8 == 0 and 0 < C <= PPM_MAX_C and 0 < Cb <= PPM_MAX_CB
            and 1 <= len(scales) <= PPM_MAX_BRANCHES and all(1 <= s <= PPM_MAX_SCALE for s in scales)
            and sum(s * s for s in scales) <= PPM_MAX_CELLS)


def ppm_unfused_forced() -> bool:
    """VKAS_PPM_UNFUSED: A/B switch, read at every call - the block takes AdaptiveAvgPools + 4 x conv_block + ResizeCat."""
    return os.environ.get('VKAS_PPM_UNFUSED') is not None


class PpmBranchesCat(Function):
    """The pooled branches of the pyramid-pooling block and their concatenation behind x (model/upernext.py:58-82) as one node:
    cat[..., :C] = x, cat[..., C + k Cb : C + (k+1) Cb] = bilinear(gelu(LN(pool_{s_k}(x) W_k^T + b_k)) -> H x W).
    ``params`` = W_k, b_k, gamma_k, beta_k per branch (fp32, as the modules hold them).  Three launches forward, four backward
    (csrc/ppm.hip); ``keep`` false: nothing is saved and the Linear output / statistics are not written.
    Parameter gradients are added onto the flat gradient views where the parameters have them (grad_sink) by the kernel that
    forms them, and go back to autograd as tensors of their own otherwise."""

    @staticmethod
    def forward(ctx, x, keep: bool, scales, *params):
        _require_cuda(x, *params)
        x = as_act(x)
        B, H, W, C = x.shape
        scales = tuple(int(s) for s in scales)
        nb = len(scales)
        if len(params) != 4 * nb or params[0].dim() != 2:
            raise ValueError('PpmBranchesCat: expected W, b, gamma, beta per scale')
        Cb = params[0].shape[0]
        if not ppm_fused_eligible(x.dtype, C, Cb, scales):
            raise ValueError(f'PpmBranchesCat: not eligible (dtype {x.dtype}, C {C}, Cb {Cb}, scales {scales})')
        for i, p in enumerate(params):
            if p.dtype != _FLOAT or tuple(p.shape) != ((Cb, C) if i % 4 == 0 else (Cb,)):
                raise ValueError(f'PpmBranchesCat: parameter {i} has shape {tuple(p.shape)} / dtype {p.dtype}')
        params = [p.contiguous() for p in params]
        sc = (ctypes.c_int * nb)(*scales)
        ptrs = (ctypes.c_void_p * (4 * nb))(*[p.data_ptr() for p in params])
        S, SS = sum(s * s for s in scales), sum(scales)
        M, dev, es, dt = B * S, x.device, x.element_size(), _dt(x)
        cat = new_act(B, H, W, C + nb * Cb, x)
        rowsum = torch.empty((B * H * SS * C,), dtype=_FLOAT, device=dev)
        act = torch.empty((M, Cb), dtype=x.dtype, device=dev)
        pooled = torch.empty((M, C), dtype=x.dtype, device=dev) if keep else None
        lin = torch.empty((M, Cb), dtype=x.dtype, device=dev) if keep else None
        stats = torch.empty((M, 2), dtype=_FLOAT, device=dev) if keep else None
        px = B * H * W
        _timed('ppm_pool_fwd_kernel', x, 0.0, px, C, 0,
               lambda: check(lib.vkas_ppm_pool_fwd(_p(x), act_ld(x), _p(cat), act_ld(cat), _p(rowsum), B, H, W, C, Cb, nb, sc, dt,
                                                   _stream()), 'ppm_pool_fwd'), 2.0 * px * C * es + 4.0 * rowsum.numel())
        _timed('ppm_rows_fwd_kernel', x, 2.0 * M * Cb * C, M, Cb, C,
               lambda: check(lib.vkas_ppm_rows_fwd(_p(rowsum), ptrs, _p(pooled), _p(lin), _p(stats), _p(act), B, H, W, C, Cb, nb, sc,
                                                   dt, _stream()), 'ppm_rows_fwd'), 4.0 * rowsum.numel() + 4.0 * nb * Cb * C)
        _timed('ppm_resize_fwd_kernel', x, 0.0, px, nb * Cb, 0,
               lambda: check(lib.vkas_ppm_resize_fwd(_p(act), _p(cat), act_ld(cat), B, H, W, C, Cb, nb, sc, dt, _stream()),
                             'ppm_resize_fwd'), float(px * nb * Cb * es))
        if keep:
            ctx.save_for_backward(pooled, lin, stats, *params)
            ctx.cfg = (B, H, W, C, Cb, scales)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        pooled, lin, stats, *params = ctx.saved_tensors
        B, H, W, C, Cb, scales = ctx.cfg
        dcat = as_act(dcat)
        nb = len(scales)
        sc = (ctypes.c_int * nb)(*scales)
        ptrs = (ctypes.c_void_p * (4 * nb))(*[p.data_ptr() for p in params])
        S, SS = sum(s * s for s in scales), sum(scales)
        M, dev, es, dt = B * S, dcat.device, dcat.element_size(), _dt(dcat)
        px = B * H * W
        tx = torch.empty((B * H * SS * Cb,), dtype=_FLOAT, device=dev)
        dz = torch.empty((M, Cb), dtype=dcat.dtype, device=dev)
        groups = lib.vkas_ppm_row_groups(B, nb, sc)
        if groups < 0:
            check(-1, 'ppm_row_groups')
        partial = torch.empty((max(groups, 1) * 2 * Cb,), dtype=_FLOAT, device=dev)
        want_dx = ctx.needs_input_grad[0]
        dp = torch.empty((M, C), dtype=_FLOAT, device=dev) if want_dx else None
        _timed('ppm_resize_bwd_x_kernel', dcat, 0.0, px, nb * Cb, 0,
               lambda: check(lib.vkas_ppm_resize_bwd_x(_p(dcat), act_ld(dcat), _p(tx), B, H, W, C, Cb, nb, sc, dt, _stream()),
                             'ppm_resize_bwd_x'), float(px * nb * Cb * es) + 4.0 * tx.numel())
        _timed('ppm_rows_bwd_kernel', dcat, 2.0 * M * Cb * C * int(want_dx), M, C, Cb,
               lambda: check(lib.vkas_ppm_rows_bwd(_p(tx), ptrs, _p(lin), _p(stats), _p(dz), _p(partial), _p(dp), B, H, W, C, Cb, nb,
                                                   sc, dt, _stream()), 'ppm_rows_bwd'),
               4.0 * tx.numel() + 4.0 * nb * Cb * C + 4.0 * M * C * int(want_dx))
        # every parameter gradient has one writer in the kernel: it adds onto the flat gradient view where there is one (no
        # delivery launch), and fills a tensor of its own otherwise (never a slice of the step's zero arena)
        dsts, accs, outs, sinks = [], [], [], []
        for i, p in enumerate(params):
            s = grad_sink(p) if ctx.needs_input_grad[3 + i] else None
            if s is not None and p.grad.is_contiguous() and p.grad.dtype == _FLOAT and p.grad.numel() == p.numel():
                dsts.append(p.grad)
                accs.append(1)
                outs.append(None)
                sinks.append(s)
            else:
                g = torch.empty(p.shape, dtype=_FLOAT, device=dev)
                dsts.append(g)
                accs.append(0)
                outs.append(g if ctx.needs_input_grad[3 + i] else None)
        gp = (ctypes.c_void_p * (4 * nb))(*[g.data_ptr() for g in dsts])
        ga = (ctypes.c_int * (4 * nb))(*accs)
        _timed('ppm_param_grads_kernel', dcat, 2.0 * M * Cb * C, Cb, C, M,
               lambda: check(lib.vkas_ppm_param_grads(_p(dz), _p(pooled), _p(partial), gp, ga, B, C, Cb, nb, sc, dt, _stream()),
                             'ppm_param_grads'), 4.0 * nb * Cb * C + float(M * (C + Cb) * es))
        for s in sinks:
            s[0].grad_delivered(s[1])
        dx = None
        if want_dx:
            dx = new_act(B, H, W, C, dcat)
            _timed('ppm_pool_bwd_kernel', dcat, 0.0, px, C, 0,
                   lambda: check(lib.vkas_ppm_pool_bwd(_p(dcat), act_ld(dcat), _p(dp), _p(dx), act_ld(dx), B, H, W, C, Cb, nb, sc,
                                                       dt, _stream()), 'ppm_pool_bwd'), 2.0 * px * C * es)
        return (dx, None, None, *outs)


class SplitBatch(Function):
    """x -> (x[:b0], x[b0:]) as views of one NHWC activation; backward writes the two gradients into the halves of one
    buffer (no zero-fill + add, which is what slicing through autograd would do).  Used by the merged pass schedule
    (model.forward_both): the backbone runs once on the rough and the precise batch, each neck reads its half."""

    @staticmethod
    def forward(ctx, x, b0: int):
        _require_cuda(x)
        x = as_act(x)
        ctx.meta = (tuple(x.shape), b0, x.dtype)
        return x[:b0], x[b0:]

    @staticmethod
    def backward(ctx, d0, d1):
        shape, b0, dtype = ctx.meta
        ref = d0 if d0 is not None else d1
        out = torch.empty(shape, dtype=dtype, device=ref.device)
        for part, d in ((out[:b0], d0), (out[b0:], d1)):
            if d is None:
                part.zero_()
            else:
                copy_channels(as_act(d), part)
        return out, None


class ToNchw(Function):
    """(B,H,W,Cp) activation -> (B,C,H,W) fp32 NCHW: the permute back of model/upernext.py:223 / fpn.py:183 for the
    1..4-channel head outputs."""

    @staticmethod
    def forward(ctx, x, C: int):
        _require_cuda(x)
        x = as_act(x)
        B, H, W, Cp = x.shape
        out = torch.empty((B, C, H, W), dtype=_FLOAT, device=x.device)
        check(lib.vkas_nhwc_to_nchw_f32(_p(x), act_ld(x), _p(out), B, H, W, C, _dt(x), _stream()), 'nhwc_to_nchw_f32')
        ctx.cfg = (Cp, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        Cp, dtype = ctx.cfg
        mark = g
        g = g.contiguous().float()
        B, C, H, W = g.shape
        out = torch.empty((B, H, W, Cp), dtype=dtype, device=g.device)
        check(lib.vkas_nchw_f32_to_nhwc(_p(g), _p(out), Cp, B, H, W, C, Cp,
                                        _dtc(dtype), _stream()),
              'nchw_f32_to_nhwc')
        return pass_point_sparse(mark, out), None  # a permutation of the pixels' channels


class Softplus(Function):
    """nn.Softplus() (model/adaptive_scaling.py:101,140)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.vkas_softplus_fwd(_p(x), _p(y), x.numel(), _stream()), 'softplus_fwd')
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mark = dy
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        check(lib.vkas_softplus_bwd(_p(x), _p(dy), _p(dx), x.numel(), _stream()), 'softplus_bwd')
        return pass_point_sparse(mark, dx)  # elementwise: zero gradient stays zero


_DEFERRED = []  # (pinned host tensor, event, message): device-side argument checks awaiting their verdict


def _defer_check(min_margin: torch.Tensor, message: str):
    """min_margin: 1-element int64 device tensor that is negative when the check failed."""
    host = torch.empty((1,), dtype=min_margin.dtype, pin_memory=True)
    host.copy_(min_margin, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _DEFERRED.append((host, ev, message))


def check_deferred(wait: bool = False):
    """Raise for any device-side argument check that has completed (all of them with wait=True) and failed."""
    keep = []
    for host, ev, message in _DEFERRED:
        if wait:
            ev.synchronize()
        if ev.query():
            if int(host[0]) < 0:
                _DEFERRED.clear()
                raise IndexError(message)
        else:
            keep.append((host, ev, message))
    _DEFERRED[:] = keep


def _check_loss_maps(who, preds, channels, gt_mask, gt_score, up, left):
    """Shape / device contract of the dense losses (loss_function/adaptive_scaling.py:67-86,213-231): every tensor on
    the GPU, predictions (B, c, H, W), targets (B, CH, CW) with the crop inside the map.  The kernels index with these
    numbers, so a mismatch must raise here instead of reading out of bounds."""
    B, _, H, W = preds[0].shape
    for t, c in zip(preds, channels):
        if tuple(t.shape) != (B, c, H, W):
            raise ValueError(f'{who}: prediction must be ({B}, {c}, {H}, {W}), got {tuple(t.shape)}')
    if gt_mask.dim() != 3 or gt_mask.shape[0] != B or gt_score.shape != gt_mask.shape:
        raise ValueError(f'{who}: targets must be (B={B}, CH, CW) and equal, got {tuple(gt_mask.shape)} / '
                         f'{tuple(gt_score.shape)}')
    _, CH, CW = gt_mask.shape
    if up < 0 or left < 0 or up + CH > H or left + CW > W:
        raise ValueError(f'{who}: core box (up={up}, left={left}, {CH}x{CW}) does not fit the {H}x{W} map')


class RoughLoss(Function):
    """AdaptiveScalingRoughLossFunction.__call__ (loss_function/adaptive_scaling.py:53-131), default-active terms."""

    @staticmethod
    def forward(ctx, mask_feat, height_feat, gt_mask, gt_score, up, left, cfg):
        _require_cuda(mask_feat, height_feat, gt_mask, gt_score)
        mask_feat, height_feat = mask_feat.contiguous().float(), height_feat.contiguous().float()
        gt_mask, gt_score = gt_mask.contiguous().float(), gt_score.contiguous().float()
        _check_loss_maps('RoughLoss', (mask_feat, height_feat), (1, 1), gt_mask, gt_score, up, left)
        B, _, H, W = mask_feat.shape
        _, CH, CW = gt_mask.shape
        sums = torch.empty((8,), dtype=torch.float64, device=mask_feat.device)
        loss = torch.empty((), dtype=_FLOAT, device=mask_feat.device)
        check(lib.vkas_rough_loss_fwd(_p(mask_feat), _p(height_feat), _p(gt_mask), _p(gt_score), B, H, W, up, left, CH,
                                      CW, ctypes.byref(cfg), _p(sums), _p(loss), _stream()), 'rough_loss_fwd')
        ctx.save_for_backward(mask_feat, height_feat, gt_mask, gt_score, sums)
        ctx.cfg = (up, left, cfg)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        mask_feat, height_feat, gt_mask, gt_score, sums = ctx.saved_tensors
        up, left, cfg = ctx.cfg
        B, _, H, W = mask_feat.shape
        _, CH, CW = gt_mask.shape
        dm, dh = torch.empty_like(mask_feat), torch.empty_like(height_feat)
        dloss = dloss.contiguous().float()
        check(lib.vkas_rough_loss_bwd(_p(mask_feat), _p(height_feat), _p(gt_mask), _p(gt_score), B, H, W, up, left, CH,
                                      CW, ctypes.byref(cfg), _p(sums), _p(dloss), _p(dm), _p(dh), _stream()),
              'rough_loss_bwd')
        return dm, dh, None, None, None, None, None


class PreciseLoss(Function):
    """AdaptiveScalingPreciseLossFunction.__call__ (loss_function/adaptive_scaling.py:181-346).  The terms that are off
    under the reference's default factors (:272-277 mask focal, :284-289 prob smooth-L1, :303-307 WAHR) are switched on by
    ``ex`` (_lib.PreciseLossExtraCfg).
    ``mask_feat`` (B, 1, H, W) mask logits may be None unless ``ex.mask_focal > 0``; it then receives a gradient."""

    @staticmethod
    def forward(ctx, prob, mask_feat, offset, angle, dist, gt_score, gt_mask, py, px, gt_off, gt_ang, gt_dist, up, left, cfg,
                ex):
        _require_cuda(prob, mask_feat, offset, angle, dist, gt_score, gt_mask, py, px, gt_off, gt_ang, gt_dist)
        if ex.mask_focal > 0 and mask_feat is None:
            raise ValueError('PreciseLoss: the mask focal term needs the mask feature')
        f = lambda t: t.contiguous().float()
        prob, offset, angle, dist = f(prob), f(offset), f(angle), f(dist)
        mask_feat = f(mask_feat) if mask_feat is not None else None
        gt_score, gt_mask, gt_off, gt_ang, gt_dist = f(gt_score), f(gt_mask), f(gt_off), f(gt_ang), f(gt_dist)
        py, px = py.contiguous().long(), px.contiguous().long()
        preds, channels = (prob, offset, angle, dist), (1, 2, 4, 4)
        if mask_feat is not None:
            preds, channels = preds + (mask_feat,), channels + (1,)
        _check_loss_maps('PreciseLoss', preds, channels, gt_mask, gt_score, up, left)
        B, _, H, W = prob.shape
        _, CH, CW = gt_mask.shape
        if py.dim() != 2 or py.shape[0] != B or px.shape != py.shape:
            raise ValueError(f'PreciseLoss: label points must be (B={B}, P), got {tuple(py.shape)} / {tuple(px.shape)}')
        P = py.shape[1]
        for name, t, last in (('up_left_offsets', gt_off, 2), ('corner_angles', gt_ang, 4), ('corner_distances', gt_dist, 3)):
            if tuple(t.shape) != (B, P, last):
                raise ValueError(f'PreciseLoss: {name} must be ({B}, {P}, {last}), got {tuple(t.shape)}')
        if P > 0 and not torch.cuda.is_current_stream_capturing():
            # The reference's advanced indexing raises on out-of-range label points (and wraps negative ones); a corrupt
            # batch must not train silently on the clamped pixels the kernel falls back to.  The range test runs on the
            # device and its verdict travels to pinned host memory asynchronously: reading it here would stall the
            # launch pipeline once per step, so it is examined at the NEXT loss call / check_deferred() (one step late).
            # Not while a HIP graph is being captured: a replay does not refresh the pinned verdict or its event, and
            # querying events is not allowed during a capture.  The kernels clamp the coordinates, so nothing reads out
            # of bounds.
            check_deferred()
            lim = torch.empty((1,), dtype=torch.int64, device=py.device)
            check(lib.vkas_points_margin(_p(py), _p(px), B * P, H, W, _p(lim), _stream()), 'points_margin')
            _defer_check(lim, f'PreciseLoss: label points outside the {H}x{W} map')
        sums = torch.empty((_lib.PRECISE_LOSS_SUMS,), dtype=torch.float64, device=prob.device)
        loss = torch.empty((), dtype=_FLOAT, device=prob.device)
        check(lib.vkas_precise_loss_fwd(_p(prob), _p(offset), _p(angle), _p(dist), _p(gt_score), _p(gt_mask), _p(py),
                                        _p(px), _p(gt_off), _p(gt_ang), _p(gt_dist), B, H, W, up, left, CH, CW, P,
                                        ctypes.byref(cfg), _p(mask_feat), ctypes.byref(ex), _p(sums), _p(loss),
                                        _stream()), 'precise_loss_fwd')
        ctx.save_for_backward(prob, mask_feat, offset, angle, dist, gt_score, gt_mask, py, px, gt_off, gt_ang, gt_dist, sums)
        ctx.cfg = (up, left, cfg, ex)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        prob, mask_feat, offset, angle, dist, gt_score, gt_mask, py, px, gt_off, gt_ang, gt_dist, sums = ctx.saved_tensors
        up, left, cfg, ex = ctx.cfg
        B, _, H, W = prob.shape
        _, CH, CW = gt_mask.shape
        P = py.shape[1]
        dp, do, da, dd = (torch.empty_like(t) for t in (prob, offset, angle, dist))
        dm = torch.empty_like(mask_feat) if mask_feat is not None and ex.mask_focal > 0 else None
        dloss = dloss.contiguous().float()
        check(lib.vkas_precise_loss_bwd(_p(prob), _p(offset), _p(angle), _p(dist), _p(gt_score), _p(gt_mask), _p(py),
                                        _p(px), _p(gt_off), _p(gt_ang), _p(gt_dist), B, H, W, up, left, CH, CW, P,
                                        ctypes.byref(cfg), _p(mask_feat), ctypes.byref(ex), _p(sums), _p(dloss),
                                        _p(dp), _p(do), _p(da), _p(dd), _p(dm), _stream()), 'precise_loss_bwd')
        # offset / angle / distance are read at the label points only (adaptive_scaling.py:235-262): their gradients are
        # zero elsewhere, which the heads' backward exploits
        for g in (do, da, dd):
            point_sparse(g, py, px)
        return (dp, dm, do, da, dd) + (None,) * 11


class ElementwiseLoss(Function):
    """The mean-/masked-mean-type primitive losses and dice (loss_function/{focal_with_logits,dice,l1,l2}.py) as one
    reduction kernel + finalize; gradient for ``pred`` only (targets and masks are data)."""

    @staticmethod
    def forward(ctx, pred, gt, mask, kind: int, p0: float, p1: float, eps: float):
        _require_cuda(pred, gt, mask)
        if gt.shape != pred.shape or (mask is not None and mask.shape != pred.shape):
            raise ValueError(f'loss: pred {tuple(pred.shape)}, gt {tuple(gt.shape)}'
                             + (f', mask {tuple(mask.shape)}' if mask is not None else '') + ' must have equal shapes')
        shape = pred.shape
        pred, gt = pred.contiguous().float(), gt.contiguous().float()
        mask = None if mask is None else mask.contiguous().float()
        sums = torch.empty((4,), dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=_FLOAT, device=pred.device)
        check(lib.vkas_elementwise_loss_fwd(kind, _p(pred), _p(gt), _p(mask), pred.numel(), p0, p1, eps, _p(sums), _p(loss),
                                            _stream()), 'elementwise_loss_fwd')
        ctx.save_for_backward(pred, gt, mask if mask is not None else torch.empty(0, device=pred.device), sums)
        ctx.cfg = (kind, p0, p1, eps, mask is not None, shape)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        pred, gt, mask, sums = ctx.saved_tensors
        kind, p0, p1, eps, has_mask, shape = ctx.cfg
        dpred = torch.empty_like(pred)
        dloss = dloss.contiguous().float()
        check(lib.vkas_elementwise_loss_bwd(kind, _p(pred), _p(gt), _p(mask) if has_mask else None, pred.numel(), p0, p1, eps,
                                            _p(sums), _p(dloss), _p(dpred), _stream()), 'elementwise_loss_bwd')
        return dpred.view(shape), None, None, None, None, None, None


class CrossEntropy(Function):
    """F.cross_entropy on (rows, classes) logits with class-probability targets of the same shape or int64 class
    indices (loss_function/cross_entropy_with_logits.py:16-19); mean over rows."""

    @staticmethod
    def forward(ctx, logits, target):
        _require_cuda(logits, target)
        if logits.dim() != 2:
            raise ValueError(f'cross entropy: logits must be (rows, classes), got {tuple(logits.shape)}')
        rows, classes = logits.shape
        hard = not target.is_floating_point()
        if hard:
            if tuple(target.shape) != (rows,):
                raise ValueError(f'cross entropy: class-index target must be ({rows},), got {tuple(target.shape)}')
            target = target.contiguous().long()
            if rows > 0:
                lo, hi = (int(v) for v in torch.stack([target.min(), target.max()]).tolist())
                if lo < 0 or hi >= classes:
                    raise IndexError(f'cross entropy: target class outside [0, {classes})')
        else:
            if target.shape != logits.shape:
                raise ValueError(f'cross entropy: probability target must be {tuple(logits.shape)}, got {tuple(target.shape)}')
            target = target.contiguous().float()
        logits = logits.contiguous().float()
        sums = torch.empty((4,), dtype=torch.float64, device=logits.device)
        loss = torch.empty((), dtype=_FLOAT, device=logits.device)
        check(lib.vkas_cross_entropy_fwd(_p(logits), _p(target), int(hard), rows, classes, _p(sums), _p(loss), _stream()),
              'cross_entropy_fwd')
        ctx.save_for_backward(logits, target)
        ctx.hard = hard
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target = ctx.saved_tensors
        rows, classes = logits.shape
        d = torch.empty_like(logits)
        dloss = dloss.contiguous().float()
        check(lib.vkas_cross_entropy_bwd(_p(logits), _p(target), int(ctx.hard), rows, classes, _p(dloss), _p(d), _stream()),
              'cross_entropy_bwd')
        return d, None


def char_polygons(prob: torch.Tensor, offset: torch.Tensor, angle: torch.Tensor, dist: torch.Tensor, thr: float, size,
                  scale_y: float, scale_x: float):
    """Peaks of the precise char-probability maps and their quadrilaterals (inferencing/adaptive_scaling.py:399-465,481-491,
    csrc/charpoly.hip).  prob (B,H,W), offset (B,H,W,2), angle (B,H,W,4) softmaxed, dist (B,H,W,4), fp32 on the device.
    ``size`` is scipy's maximum_filter size (a float is truncated, as scipy does); ``thr`` is compared in fp32.  Returns
    ``(count, points, probs, quads)`` as device tensors of capacity B*H*W rows - (1,) int32, (cap,3) int32 (b, y, x),
    (cap,) fp32, (cap,4,2) fp32 (y, x) - of which the first ``count`` are valid, in (b, y, x) order.  Never synchronises,
    so it can be captured into a HIP graph."""
    if prob.dim() != 3:
        raise ValueError(f'char_polygons: prob must be (B, H, W), got {tuple(prob.shape)}')
    B, H, W = prob.shape
    for name, t, c in (('offset', offset, 2), ('angle', angle, 4), ('dist', dist, 4)):
        if tuple(t.shape) != (B, H, W, c):
            raise ValueError(f'char_polygons: {name} must be {(B, H, W, c)}, got {tuple(t.shape)}')
    for name, t in (('prob', prob), ('offset', offset), ('angle', angle), ('dist', dist)):
        if t.dtype != torch.float32:
            raise ValueError(f'char_polygons: {name} must be float32, got {t.dtype}')
    if H < 1 or W < 1:
        raise ValueError(f'char_polygons: empty map {(H, W)}')
    isize = int(size)
    if isize < 1:
        raise ValueError(f'char_polygons: maximum filter size {size} truncates to {isize} (< 1)')
    if B * H * W >= 1 << 31:
        raise ValueError(f'char_polygons: B*H*W = {B * H * W} must stay below 2^31')
    _require_cuda(prob, offset, angle, dist)
    prob, offset, angle, dist = (t.contiguous() for t in (prob, offset, angle, dist))
    cap, dev = B * H * W, prob.device
    ws = _workspace('char_polygons', lib.vkas_char_polygons_workspace_bytes(B, H, W, isize), dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    points = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    probs = torch.empty((cap,), dtype=_FLOAT, device=dev)
    quads = torch.empty((cap, 4, 2), dtype=_FLOAT, device=dev)
    if cap == 0:
        return count.zero_(), points, probs, quads
    check(lib.vkas_char_polygons(_p(prob), _p(offset), _p(angle), _p(dist), B, H, W, isize, float(thr), float(scale_y),
                                 float(scale_x), _p(ws), ws.numel(), _p(count), _p(points), _p(probs), _p(quads), _stream()),
          'char_polygons')
    return count, points, probs, quads


# ---- the checks the ops over quad row tables share: every ValueError comes before the device check -------------------------

def _row_table(who: str, side: str, rows: torch.Tensor, count: torch.Tensor, words: int = 16) -> Tuple[int, int]:
    """one (B, K, words) int32 row table and its (B,) int32 count -> B, K; ``side`` is '', 'gt_' or 'pred_'"""
    if rows.dim() != 3 or rows.shape[2] != words:
        raise ValueError(f'{who}: {side}rows must be (B, K, {words}), got {tuple(rows.shape)}')
    B, K = int(rows.shape[0]), int(rows.shape[1])
    if count.shape != (B,):
        raise ValueError(f'{who}: {side}count must be {(B,)}, got {tuple(count.shape)}')
    if rows.dtype != torch.int32 or count.dtype != torch.int32:
        raise ValueError(f'{who}: {side}rows and {side}count must be int32, got {rows.dtype} and {count.dtype}')
    return B, K


def _row_values(who: str, name: str, t: Optional[torch.Tensor], shape, dtype):
    """an optional table with one value per row (``gt_care``, ``probs``)"""
    if t is not None and (t.shape != shape or t.dtype != dtype):
        raise ValueError(f'{who}: {name} must be a {shape} {dtype} tensor, got {tuple(t.shape)} {t.dtype}')


def _one_device(who: str, *tensors, also=None):
    """``tensors`` (None allowed) and ``also`` are on one GPU -> ``tensors``, contiguous"""
    dev = tensors[0].device
    for t in tensors + (also,):
        if t is not None:
            _require_cuda(t)
            if t.device != dev:
                raise ValueError(f'{who}: all tensors must be on one device')
    return tuple(None if t is None else t.contiguous() for t in tensors)


def _quad_limits(who: str, B: int, names: str, sizes, max_pairs, rounds, rounds_tail=(), T: int = 1) -> int:
    """What the kernels over match rows hold a call to - 1..8192 rows a side, B * T workgroups, a (B, *rounds_tail)
    ``rounds`` - and the one place ``max_pairs`` is resolved: 4 rows' worth by default, B * max_pairs below 2^31."""
    if min(sizes) < 1 or max(sizes) > 8192:
        raise ValueError(f'{who}: {names} = {sizes} must lie in 1..8192')
    if B * T > 65535:
        raise ValueError(f'{who}: B = {B} above 65535' if T == 1 else f'{who}: B*T = {B * T} above 65535')
    max_pairs = 4 * max(sizes) if max_pairs is None else int(max_pairs)
    if max_pairs < 0 or B * max_pairs >= 1 << 31:
        raise ValueError(f'{who}: max_pairs = {max_pairs} must be >= 0 and B*max_pairs below 2^31')
    if rounds is not None and (rounds.shape != (B,) + rounds_tail or rounds.dtype != torch.int32 or not rounds.is_contiguous()):
        raise ValueError(f'{who}: rounds must be a contiguous {(B,) + rounds_tail} int32 tensor')
    return max_pairs


def _quad_tables(who: str, gt_rows, gt_count, pred_rows, pred_count, max_pairs, rounds, rounds_tail=(), gt_care=None,
                 probs=None, T: int = 1):
    """The tables of a two-sided call: match rows and counts, optional ``gt_care`` (B, M) uint8 and ``probs`` (B, N) float32
    -> ``(gt_rows, gt_count, pred_rows, pred_count, gt_care, probs)`` contiguous on one GPU, ``B, M, N, max_pairs``."""
    B, M = _row_table(who, 'gt_', gt_rows, gt_count)
    Bp, N = _row_table(who, 'pred_', pred_rows, pred_count)
    if Bp != B:
        raise ValueError(f'{who}: {B} images of annotations against {Bp} of predictions')
    _row_values(who, 'gt_care', gt_care, (B, M), torch.uint8)
    _row_values(who, 'probs', probs, (B, N), torch.float32)
    max_pairs = _quad_limits(who, B, '(M, N)', (M, N), max_pairs, rounds, rounds_tail, T)
    return _one_device(who, gt_rows, gt_count, pred_rows, pred_count, gt_care, probs, also=rounds), B, M, N, max_pairs


def _quad_table(who: str, rows, count, probs=None, max_pairs=0, rounds=None):
    """The one-sided form -> ``(rows, count, probs)`` contiguous on one GPU, ``B, K, max_pairs``."""
    B, K = _row_table(who, '', rows, count)
    _row_values(who, 'probs', probs, (B, K), torch.float32)
    max_pairs = _quad_limits(who, B, '(K,)', (K,), max_pairs, rounds)
    return _one_device(who, rows, count, probs, also=rounds), B, K, max_pairs


def char_label_maps(rows: torch.Tensor, count: torch.Tensor, h: int, w: int, box, sigma: float = 0.5,
                    with_owner: bool = False, with_height: bool = True, with_score: bool = True):
    """Training label maps from character quadrilaterals on the device (csrc/labels.hip; the rule and the host oracle:
    dataset/labels.py).  ``rows`` (B, K, 20) int32 quad rows and ``count`` (B,) int32 on the device, the (h, w) map, the
    inclusive core ``box`` (``.up/.down/.left/.right`` or a 4-tuple in that order).  Returns ``(owner, mask, height, score)``,
    each (B, CH, CW) cropped to the box - int32 ``index + 1`` (0 = none), and fp32 ``owner != 0``, the owner's height, ``exp(-a)``
    of the owner - with None for an output that was not asked for.  One launch; never synchronises, so it can be captured
    into a HIP graph."""
    B, K = _row_table('char_label_maps', '', rows, count, words=20)
    up, down, left, right = (int(v) for v in (box if isinstance(box, (tuple, list)) else
                                              (box.up, box.down, box.left, box.right)))
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'char_label_maps: empty map {(h, w)}')
    if not (0 <= up <= down < h and 0 <= left <= right < w):
        raise ValueError(f'char_label_maps: core box {(up, down, left, right)} outside the {(h, w)} map')
    if B > 65535:
        raise ValueError(f'char_label_maps: B = {B} above 65535')
    if B * h * w >= 1 << 31:
        raise ValueError(f'char_label_maps: B*h*w = {B * h * w} must stay below 2^31')
    sigma = float(sigma)
    if not (sigma > 0.0 and sigma < float('inf')):
        raise ValueError(f'char_label_maps: sigma must be finite and positive, got {sigma}')
    rows, count = _one_device('char_label_maps', rows, count)
    CH, CW, dev = down - up + 1, right - left + 1, rows.device
    new = lambda want, dtype: torch.empty((B, CH, CW), dtype=dtype, device=dev) if want else None
    owner, mask = new(with_owner, torch.int32), new(True, _FLOAT)
    height, score = new(with_height, _FLOAT), new(with_score, _FLOAT)
    if B:
        check(lib.vkas_char_label_maps(_p(rows), _p(count), B, K, h, w, up, left, CH, CW, 1.0 / (2.0 * sigma * sigma),
                                       _p(owner), _p(mask), _p(height), _p(score), _stream()), 'char_label_maps')
    return owner, mask, height, score


def match_quads(gt_rows: torch.Tensor, gt_count: torch.Tensor, pred_rows: torch.Tensor, pred_count: torch.Tensor,
                iou_thr: float = 0.5, max_pairs: Optional[int] = None, rounds: Optional[torch.Tensor] = None):
    """Predicted character quadrilaterals matched one to one to annotated ones by IoU on the device (csrc/quadmatch.hip; the
    rule and the host oracles: inferencing/evaluation.py).  ``gt_rows`` (B, M, 16) / ``gt_count`` (B,) and ``pred_rows``
    (B, N, 16) / ``pred_count`` (B,): int32 match rows (``inferencing.match_rows``) and counts on the device; M and N at most
    8192.  ``max_pairs`` is the capacity for stored candidates (pairs with iou >= ``iou_thr``) per image, 4 * max(M, N) by
    default.  Returns ``(gt_match, pred_match, gt_iou, stats)`` - (B, M) int32 pred index or -1, (B, N) int32 gt index or -1,
    (B, M) float64 (0 where unmatched), (B, 6) int64 ``tp, n_gt, n_pred, pairs, candidates, status``.  An image with more
    candidates than ``max_pairs`` keeps its true ``pairs`` and ``candidates`` and gets ``status = 1``, every match -1 and
    ``tp = 0``.  ``rounds``, if given, is a (B,) int32 device tensor that receives the matching rounds of each image.  Four
    launches; never synchronises, so it can be captured into a HIP graph."""
    from .inferencing.evaluation import check_iou_thr  # the rule's own check, stated once
    iou_thr = check_iou_thr(iou_thr, 'match_quads')
    (gt_rows, gt_count, pred_rows, pred_count, _, _), B, M, N, max_pairs = _quad_tables(
        'match_quads', gt_rows, gt_count, pred_rows, pred_count, max_pairs, rounds)
    dev = gt_rows.device
    gt_match = torch.empty((B, M), dtype=torch.int32, device=dev)
    pred_match = torch.empty((B, N), dtype=torch.int32, device=dev)
    gt_iou = torch.empty((B, M), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 6), dtype=torch.int64, device=dev)
    if B:
        ws = _workspace('match_quads', lib.vkas_quad_match_workspace_bytes(B, M, N, max_pairs), dev)
        check(lib.vkas_quad_match(_p(gt_rows), _p(gt_count), _p(pred_rows), _p(pred_count), B, M, N, iou_thr, max_pairs, _p(ws),
                                  ws.numel(), _p(gt_match), _p(pred_match), _p(gt_iou), _p(stats), _p(rounds), _stream()),
              'match_quads')
    return gt_match, pred_match, gt_iou, stats


def match_quads_ranked(gt_rows: torch.Tensor, gt_count: torch.Tensor, gt_care: Optional[torch.Tensor],
                       pred_rows: torch.Tensor, pred_count: torch.Tensor, probs: torch.Tensor, iou_thrs,
                       cover_thr: float = 0.5, max_pairs: Optional[int] = None, rounds: Optional[torch.Tensor] = None):
    """Predicted character quadrilaterals matched to annotated ones in score order at T IoU thresholds, with don't-care
    annotations, on the device (csrc/quadmatch.hip; the rule and the host oracles: inferencing/ranking.py).  ``gt_rows``
    (B, M, 16) / ``gt_count`` (B,) and ``pred_rows`` (B, N, 16) / ``pred_count`` (B,): int32 match rows and counts;
    ``gt_care`` (B, M) uint8 with 0 = don't care, or None = every annotation counts; ``probs`` (B, N) float32; all on the
    device.  ``iou_thrs``: T host floats, strictly ascending in (0, 1], T at most 16; ``cover_thr`` in (0, 1].  ``max_pairs``
    is the capacity for stored candidates (care pairs with iou >= ``iou_thrs[0]``) per image, 4 * max(M, N) by default.
    Returns ``(pred_match (B, T, N) int32, pred_state (B, T, N) uint8, gt_match (B, T, M) int32, pred_iou (B, T, N) float64,
    covered (B, N) uint8, stats (B, T, 8) int64, dc_stats (B, 3) int64)`` with states 0 ABSENT, 1 TP, 2 FP, 3 IGNORED,
    ``stats`` = tp, fp, ignored, n_gt, n_pred, pairs, candidates, status and ``dc_stats`` = n_dc, dc_pairs, n_covered.  An
    image over the capacity keeps its true counts and gets ``status = 1``, every state 0 and every match -1.  ``rounds``, if
    given, is a (B, T) int32 device tensor that receives the rounds.  Four launches; never synchronises, so it can be captured
    into a HIP graph."""
    what = 'match_quads_ranked'
    from .inferencing.ranking import check_thresholds  # the rule's own check, stated once
    thrs, cover_thr = check_thresholds(iou_thrs, cover_thr)
    T = len(thrs)
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, probs), B, M, N, max_pairs = _quad_tables(
        what, gt_rows, gt_count, pred_rows, pred_count, max_pairs, rounds, (T,), gt_care, probs, T)
    dev = gt_rows.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    pred_match, pred_state = new((B, T, N), torch.int32), new((B, T, N), torch.uint8)
    gt_match, pred_iou = new((B, T, M), torch.int32), new((B, T, N), torch.float64)
    covered, stats, dc_stats = new((B, N), torch.uint8), new((B, T, 8), torch.int64), new((B, 3), torch.int64)
    if B:
        ws = _workspace(what, lib.vkas_quad_match_ranked_workspace_bytes(B, M, N, T, max_pairs), dev)
        host_thrs = (ctypes.c_double * T)(*thrs)  # read by the launcher before it returns
        check(lib.vkas_quad_match_ranked(_p(gt_rows), _p(gt_count), _p(gt_care), _p(pred_rows), _p(pred_count), _p(probs), B, M,
                                         N, ctypes.cast(host_thrs, ctypes.c_void_p), T, cover_thr, max_pairs, _p(ws),
                                         ws.numel(), _p(pred_match), _p(pred_state), _p(gt_match), _p(pred_iou), _p(covered),
                                         _p(stats), _p(dc_stats), _p(rounds), _stream()), what)
    return pred_match, pred_state, gt_match, pred_iou, covered, stats, dc_stats


def match_lines(gt_rows: torch.Tensor, gt_count: torch.Tensor, gt_care: Optional[torch.Tensor], pred_rows: torch.Tensor,
                pred_count: torch.Tensor, recall_thr: float = 0.8, precision_thr: float = 0.4, cover_thr: float = 0.5,
                max_pairs: Optional[int] = None, rounds: Optional[torch.Tensor] = None):
    """Detected text lines scored against annotated ones with one-to-one matches, splits and merges on the device
    (csrc/linematch.hip; the rule and the host oracles: inferencing/line_evaluation.py).  ``gt_rows`` (B, M, 16) / ``gt_count``
    (B,) and ``pred_rows`` (B, N, 16) / ``pred_count`` (B,): int32 match rows and counts; ``gt_care`` (B, M) uint8 with 0 =
    don't care, or None = every annotation counts; all on the device, M and N at most 8192.  ``recall_thr`` and
    ``precision_thr`` in (0, 1] become Q8 integers by ``rint(x * 256)``; ``cover_thr`` in (0, 1].  ``max_pairs`` is the capacity
    for stored candidates per image, 4 * max(M, N) by default.  Returns ``(gt_kind (B, M) uint8, gt_group (B, M) int32,
    pred_kind (B, N) uint8, pred_group (B, N) int32, stats (B, 16) int64)`` as the rule lays them out.  An image over the
    capacity keeps its true counts and gets ``status = 1`` and no match.  ``rounds``, if given, is a (B, 2) int32 device tensor
    that receives the split and merge rounds.  Four launches; allocates only its outputs and workspace and never
    synchronises, so it can be captured into a HIP graph."""
    what = 'match_lines'
    from .inferencing.line_evaluation import check_line_thresholds  # the rule's own check, stated once
    tr_q8, tp_q8, cover_thr = check_line_thresholds(recall_thr, precision_thr, cover_thr)
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, _), B, M, N, max_pairs = _quad_tables(
        what, gt_rows, gt_count, pred_rows, pred_count, max_pairs, rounds, (2,), gt_care)
    dev = gt_rows.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    gt_kind, gt_group = new((B, M), torch.uint8), new((B, M), torch.int32)
    pred_kind, pred_group = new((B, N), torch.uint8), new((B, N), torch.int32)
    stats = new((B, 16), torch.int64)
    if B:
        ws = _workspace(what, lib.vkas_line_match_workspace_bytes(B, M, N, max_pairs), dev)
        check(lib.vkas_line_match(_p(gt_rows), _p(gt_count), _p(gt_care), _p(pred_rows), _p(pred_count), B, M, N, tr_q8, tp_q8,
                                  cover_thr, max_pairs, _p(ws), ws.numel(), _p(gt_kind), _p(gt_group), _p(pred_kind),
                                  _p(pred_group), _p(stats), _p(rounds), _stream()), what)
    return gt_kind, gt_group, pred_kind, pred_group, stats


def match_ribbons(gt_rows: torch.Tensor, gt_count: torch.Tensor, gt_care: Optional[torch.Tensor], gt_segs: torch.Tensor,
                  pred_rows: torch.Tensor, pred_count: torch.Tensor, pred_segs: torch.Tensor, recall_thr: float = 0.8,
                  precision_thr: float = 0.4, cover_thr: float = 0.5, max_pairs: Optional[int] = None,
                  rounds: Optional[torch.Tensor] = None):
    """Curved text lines scored as ribbons of quads on the device (csrc/ribbonmatch.hip; the rule and the host oracles:
    inferencing/ribbon_evaluation.py).  ``gt_rows`` (B, M, 16) / ``gt_count`` (B,) and ``pred_rows`` (B, N, 16) / ``pred_count``
    (B,): int32 ribbon rows and counts; ``gt_segs`` (B, Sg, 16) and ``pred_segs`` (B, Sp, 16): the int32 segment tables the
    ribbon rows index (``inferencing.ribbon_tables``), Sg and Sp in 1..2^21; ``gt_care`` (B, M) uint8 with 0 = don't care, or
    None; all on the device.  Thresholds, ``max_pairs``, ``rounds`` and the five results are those of ``match_lines``.  Four
    launches; allocates only its outputs and workspace and never synchronises, so it can be captured into a HIP graph."""
    what = 'match_ribbons'
    from .inferencing.line_evaluation import check_line_thresholds  # the rule's own check, stated once
    tr_q8, tp_q8, cover_thr = check_line_thresholds(recall_thr, precision_thr, cover_thr)
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, _), B, M, N, max_pairs = _quad_tables(
        what, gt_rows, gt_count, pred_rows, pred_count, max_pairs, rounds, (2,), gt_care)
    for name, segs in (('gt_segs', gt_segs), ('pred_segs', pred_segs)):
        if segs.dim() != 3 or segs.shape[0] != B or segs.shape[2] != 16 or segs.dtype != torch.int32:
            raise ValueError(f'{what}: {name} must be a ({B}, S, 16) int32 tensor, got {tuple(segs.shape)} {segs.dtype}')
        if not 1 <= segs.shape[1] <= 1 << 21:
            raise ValueError(f'{what}: {name} holds {segs.shape[1]} rows per image, outside 1..2^21')
    gt_segs, pred_segs = _one_device(what, gt_segs, pred_segs, also=gt_rows)
    dev = gt_rows.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    gt_kind, gt_group = new((B, M), torch.uint8), new((B, M), torch.int32)
    pred_kind, pred_group = new((B, N), torch.uint8), new((B, N), torch.int32)
    stats = new((B, 16), torch.int64)
    if B:
        ws = _workspace(what, lib.vkas_ribbon_match_workspace_bytes(B, M, N, max_pairs), dev)
        check(lib.vkas_ribbon_match(_p(gt_rows), _p(gt_count), _p(gt_care), _p(gt_segs), int(gt_segs.shape[1]), _p(pred_rows),
                                    _p(pred_count), _p(pred_segs), int(pred_segs.shape[1]), B, M, N, tr_q8, tp_q8, cover_thr,
                                    max_pairs, _p(ws), ws.numel(), _p(gt_kind), _p(gt_group), _p(pred_kind), _p(pred_group),
                                    _p(stats), _p(rounds), _stream()), what)
    return gt_kind, gt_group, pred_kind, pred_group, stats


def quad_rows(quads: torch.Tensor, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``inferencing.match_rows`` on the device (csrc/quadmatch.hip): ``quads`` (B, K, 4, 2) float64 ``(y, x)`` corners and an
    optional ``valid`` (B, K) uint8 on the device -> (B, K, 16) int32 match rows, equal to the host's on every input (an
    invalid quad gets a zero row).  One launch; never synchronises, so it can be captured into a HIP graph."""
    if quads.dim() != 4 or tuple(quads.shape[2:]) != (4, 2):
        raise ValueError(f'quad_rows: quads must be (B, K, 4, 2), got {tuple(quads.shape)}')
    if quads.dtype != torch.float64:
        raise ValueError(f'quad_rows: quads must be float64, got {quads.dtype}')
    B, K = int(quads.shape[0]), int(quads.shape[1])
    if B * K >= 1 << 27:
        raise ValueError(f'quad_rows: B*K = {B * K} must stay below 2^27')
    if valid is not None and (tuple(valid.shape) != (B, K) or valid.dtype != torch.uint8):
        raise ValueError(f'quad_rows: valid must be a {(B, K)} uint8 tensor, got {tuple(valid.shape)} {valid.dtype}')
    tensors = (quads,) + (() if valid is None else (valid,))
    _require_cuda(*tensors)
    if any(t.device != quads.device for t in tensors):
        raise ValueError('quad_rows: all tensors must be on one device')
    quads = quads.contiguous()
    valid = None if valid is None else valid.contiguous()
    rows = torch.empty((B, K, 16), dtype=torch.int32, device=quads.device)
    if B * K:
        check(lib.vkas_quad_rows(_p(quads), _p(valid), B, K, _p(rows), _stream()), 'quad_rows')
    return rows


def nms_quads(rows: torch.Tensor, count: torch.Tensor, probs: torch.Tensor, iou_thr: float = 0.5,
              max_pairs: Optional[int] = None, rounds: Optional[torch.Tensor] = None):
    """Greedy non-maximum suppression of character quadrilaterals by IoU on the device (csrc/quadmatch.hip; the rule and the
    host oracle ``nms_quads_host``: inferencing/nms.py).  ``rows`` (B, K, 16) int32 match rows (``ops.quad_rows``), ``count``
    (B,) int32, ``probs`` (B, K) float32, all on the device; K at most 8192.  ``max_pairs`` is the capacity for stored
    candidates (outranking pairs with iou >= ``iou_thr``) per image, 4 * K by default.  Returns ``(keep, suppressor, stats)`` -
    (B, K) uint8 (0 beyond the count), (B, K) int32 (the highest-ranked kept neighbour of a suppressed quad, else -1),
    (B, 6) int64 ``kept, n, n_valid, pairs, candidates, status``.  An image with more candidates than ``max_pairs`` keeps its
    true ``pairs`` and ``candidates`` and gets ``status = 1``, every quad within the count kept and every suppressor -1.
    ``rounds``, if given, is a (B,) int32 device tensor that receives the rounds of each image.  Four launches; never
    synchronises, so it can be captured into a HIP graph."""
    from .inferencing.evaluation import check_iou_thr  # the rule's own check, stated once
    iou_thr = check_iou_thr(iou_thr, 'nms_quads')
    (rows, count, probs), B, K, max_pairs = _quad_table('nms_quads', rows, count, probs, max_pairs, rounds)
    dev = rows.device
    keep = torch.empty((B, K), dtype=torch.uint8, device=dev)
    suppressor = torch.empty((B, K), dtype=torch.int32, device=dev)
    stats = torch.empty((B, 6), dtype=torch.int64, device=dev)
    if B:
        ws = _workspace('nms_quads', lib.vkas_quad_nms_workspace_bytes(B, K, max_pairs), dev)
        check(lib.vkas_quad_nms(_p(rows), _p(count), _p(probs), B, K, iou_thr, max_pairs, _p(ws), ws.numel(), _p(keep),
                                _p(suppressor), _p(stats), _p(rounds), _stream()), 'nms_quads')
    return keep, suppressor, stats


def quad_lines(rows: torch.Tensor, count: torch.Tensor, gap: float = 1.5, cross: float = 0.5, height_ratio: float = 2.0):
    """Grouping of character quadrilaterals into text lines on the device (csrc/quadlines.hip; the rule and the host oracle
    ``quad_lines_host``: inferencing/lines.py).  ``rows`` (B, K, 16) int32 match rows (``ops.quad_rows``), ``count`` (B,) int32,
    both on the device; K at most 8192.  ``gap``, ``cross`` and ``height_ratio`` are in character heights and become Q4
    integers by ``rint(x * 16)``: 1..4096, 1..4096 and 16..256.  Returns ``(line, order, table, stats)`` - (B, K) int32 (the
    line of each quad, -1 for one that takes no part), (B, K) int32 (the member indices line after line in reading order,
    then -1), (B, K, 8) int64 rows ``start, size, U_y, U_x, a_min, a_max, b_min, b_max`` (zero from the image's line count
    on), (B, 4) int64 ``n, n_part, links, lines``.  K table rows is the exact worst case: there is no overflow path.  Eight
    launches; never synchronises, so it can be captured into a HIP graph."""
    from .inferencing.lines import line_params  # the rule's own check, stated once
    gap_q4, cross_q4, ratio_q4 = line_params(gap, cross, height_ratio)
    (rows, count, _), B, K, _ = _quad_table('quad_lines', rows, count)  # no candidates: no capacity to check
    dev = rows.device
    line = torch.empty((B, K), dtype=torch.int32, device=dev)
    order = torch.empty((B, K), dtype=torch.int32, device=dev)
    table = torch.empty((B, K, 8), dtype=torch.int64, device=dev)
    stats = torch.empty((B, 4), dtype=torch.int64, device=dev)
    if B:
        ws = _workspace('quad_lines', lib.vkas_quad_lines_workspace_bytes(B, K), dev)
        check(lib.vkas_quad_lines(_p(rows), _p(count), B, K, gap_q4, cross_q4, ratio_q4, _p(ws), ws.numel(), _p(line),
                                  _p(order), _p(table), _p(stats), _stream()), 'quad_lines')
    return line, order, table, stats


def text_regions(mask: torch.Tensor, height: torch.Tensor, max_regions: int):
    """Text regions of the rough maps and the median character height of each (the step between the two passes,
    inferencing/adaptive_scaling.py:190-279 restated on pixels, csrc/regions.hip).  mask (B,H,W) uint8 and height (B,H,W)
    fp32 on the device, as ``vkas_rough_postprocess`` writes them.  A region is an 8-connected component of ``mask != 0``;
    the regions of each image are numbered 1..N by their first pixel in row-major order.  Returns device tensors ``(count,
    labels, boxes, areas, valid, medians)`` - (B,) int32 true region counts, (B,H,W) int32 labels (0 = background), and with
    R = ``max_regions`` rows per image (row r-1 for region r; zero beyond an image's count): (B,R,4) int32 inclusive (y0, x0,
    y1, x1), (B,R) int32 pixel counts, (B,R) int32 counts of pixels with height > 0, (B,R) fp32 exact medians of those
    heights (0 without any).  An image with more than R regions keeps its true count and labels and fills R rows.  Never
    synchronises, so it can be captured into a HIP graph."""
    if mask.dim() != 3:
        raise ValueError(f'text_regions: mask must be (B, H, W), got {tuple(mask.shape)}')
    B, H, W = mask.shape
    if tuple(height.shape) != (B, H, W):
        raise ValueError(f'text_regions: height must be {(B, H, W)}, got {tuple(height.shape)}')
    if mask.dtype != torch.uint8:
        raise ValueError(f'text_regions: mask must be uint8, got {mask.dtype}')
    if height.dtype != torch.float32:
        raise ValueError(f'text_regions: height must be float32, got {height.dtype}')
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f'text_regions: empty maps {(B, H, W)}')
    R = int(max_regions)
    if R != max_regions or R < 1:
        raise ValueError(f'text_regions: max_regions must be an integer >= 1, got {max_regions}')
    if B * H * W >= 1 << 31:
        raise ValueError(f'text_regions: B*H*W = {B * H * W} must stay below 2^31')
    _require_cuda(mask, height)
    if mask.device != height.device:
        raise ValueError(f'text_regions: mask is on {mask.device}, height on {height.device}')
    mask, height = mask.contiguous(), height.contiguous()
    dev = mask.device
    ws = _workspace('text_regions', lib.vkas_text_regions_workspace_bytes(B, H, W, R), dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    boxes = torch.empty((B, R, 4), dtype=torch.int32, device=dev)
    areas = torch.empty((B, R), dtype=torch.int32, device=dev)
    valid = torch.empty((B, R), dtype=torch.int32, device=dev)
    medians = torch.empty((B, R), dtype=_FLOAT, device=dev)
    check(lib.vkas_text_regions(_p(mask), _p(height), B, H, W, R, _p(ws), ws.numel(), _p(count), _p(labels), _p(boxes),
                                _p(areas), _p(valid), _p(medians), _stream()), 'text_regions')
    return count, labels, boxes, areas, valid, medians


_PACK_DIM_MAX = 32768


def _pack_sides(who: str, name: str, shape, fdf: int = 1) -> Tuple[int, int]:
    """``shape`` as the (height, width) of ``name`` - a source, a page, or a label page at ``1/fdf`` of its page: both sides
    are at least 1 and, times ``fdf``, at most ``_PACK_DIM_MAX`` (csrc/respack.hip's DIM_MAX)."""
    try:
        H, W = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: {name} must be (height, width), got {shape!r}') from None
    if H < 1 or W < 1:
        raise ValueError(f'{who}: empty {name} {(H, W)}')
    if max(H, W) * fdf > _PACK_DIM_MAX:
        raise ValueError(f'{who}: {name} {(H * fdf, W * fdf)} sides must not exceed {_PACK_DIM_MAX}')
    return H, W


def _pack_image(who: str, name: str, t: torch.Tensor) -> Tuple[int, int]:
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f'{who}: {name} must be (H, W, 3), got {tuple(t.shape)}')
    if t.dtype != torch.uint8:
        raise ValueError(f'{who}: {name} must be uint8, got {t.dtype}')
    return _pack_sides(who, name, t.shape[:2])


def _pack_factor(who: str, fdf) -> int:
    if fdf != int(fdf) or not 1 <= int(fdf) <= 64:
        raise ValueError(f'{who}: fdf must be an integer in [1, 64], got {fdf}')
    return int(fdf)


def _pack_table(who: str, name: str, t, shape, dtype: str, device, validate: bool, check=None):
    """A table of a pack - a numpy array, a CPU tensor or a device tensor of ``shape`` (an entry that is no int: any size) and
    ``dtype`` - as a contiguous tensor on ``device``, and its host array (None for a trusted device table).  Host data is
    always checked - ``check(array)`` returns what is uploaded - and uploaded; device data must be on ``device`` and is copied
    to the host for the same check only when ``validate`` - a synchronisation -, else trusted (a captured graph's static
    table: the kernels skip a row that is out of range, but overlapping destinations give an unspecified winner)."""
    import numpy as np
    if not isinstance(t, torch.Tensor):
        t = np.asarray(t)
    if len(t.shape) != len(shape) or any(isinstance(w, int) and v != w for v, w in zip(t.shape, shape)):
        raise ValueError(f'{who}: {name} must be {shape}, got {tuple(t.shape)}'.replace("'", ''))  # ('n', 8) -> (n, 8)
    if str(t.dtype).replace('torch.', '') != dtype:
        raise ValueError(f'{who}: {name} must be {dtype}, got {t.dtype}')
    if isinstance(t, torch.Tensor) and t.is_cuda:
        if t.device != device:
            raise ValueError(f'{who}: {name} is on {t.device}, not on {device}')
        a = t.detach().cpu().numpy() if validate else None
        if a is not None and check is not None:
            check(a)
        return t.contiguous(), a
    a = t.numpy() if isinstance(t, torch.Tensor) else t
    if check is not None:
        a = check(a)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device, non_blocking=True), a


def _placements(who: str, placements, src_shape, page_shape, device, validate: bool) -> torch.Tensor:
    from .inferencing.packing import check_placements  # sides, bounds, disjoint destinations
    return _pack_table(who, 'placements', placements, ('n', 8), 'int32', device, validate,
                       lambda a: check_placements(a, src_shape, page_shape))[0]


def _warps(who: str, warps, page_shape, device, validate: bool) -> torch.Tensor:
    from .inferencing.packing import check_warps  # bounds, destinations inside the page and pairwise disjoint
    return _pack_table(who, 'warps', warps, ('K', 12), 'int64', device, validate, lambda a: check_warps(a, page_shape))[0]


def _label_args(who: str, labels: torch.Tensor, valid_shape, image_shape, out_shape, fdf):
    """The geometry of a label pack, checked: ``(Hl, Wl, vh, vw, Hs, Ws, Hq, Wq, fdf)``."""
    if labels.dim() != 2:
        raise ValueError(f'{who}: labels must be (H, W), got {tuple(labels.shape)}')
    if labels.dtype != torch.int32:
        raise ValueError(f'{who}: labels must be int32, got {labels.dtype}')
    Hl, Wl = _pack_sides(who, 'labels', labels.shape)
    vh, vw = (int(v) for v in valid_shape)
    if not (1 <= vh <= Hl and 1 <= vw <= Wl):
        raise ValueError(f'{who}: valid_shape {(vh, vw)} does not fit the {(Hl, Wl)} label map')
    fdf = _pack_factor(who, fdf)
    Hs, Ws = _pack_sides(who, 'image_shape', image_shape)
    Hq, Wq = _pack_sides(who, 'label page', out_shape, fdf)
    return Hl, Wl, vh, vw, Hs, Ws, Hq, Wq, fdf


def _region_ids(who: str, region_ids, n: int, device) -> torch.Tensor:
    """The (n,) int32 region ids on ``device``; host ids are checked to start at 1, device ids are trusted."""
    if not isinstance(region_ids, torch.Tensor):
        import numpy as np
        region_ids = torch.from_numpy(np.ascontiguousarray(np.asarray(region_ids)))
    if region_ids.dim() != 1 or region_ids.shape[0] != n:
        raise ValueError(f'{who}: region_ids must be ({n},), got {tuple(region_ids.shape)}')
    if region_ids.dtype != torch.int32:
        raise ValueError(f'{who}: region_ids must be int32, got {region_ids.dtype}')
    if not region_ids.is_cuda and n and int(region_ids.min()) < 1:
        raise ValueError(f'{who}: region ids start at 1 (0 is "no region")')
    return region_ids.to(device, non_blocking=True).contiguous()


def resample_pack_u8(src: torch.Tensor, placements, page_shape: Tuple[int, int], validate: bool = True,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Crops, rescales and packs rectangles of one image into a page (the step between the two passes,
    inferencing/adaptive_scaling.py:190-293 restated on pixels, csrc/respack.hip).  src (Hs,Ws,3) uint8 on the device;
    ``placements`` (n,8) int32 rows (sy, sx, sh, sw, dy, dx, dh, dw), host or device (see ``_pack_table``); returns the
    (Hp,Wp,3) uint8 page (``out`` if given): the resampled pixels inside the placements - the integer rule of
    inferencing/packing.py, equal to ``resample_host`` byte for byte - and zero elsewhere.  One launch; with a device table
    and ``validate=False`` it never synchronises, so it can be captured into a HIP graph."""
    Hs, Ws = _pack_image('resample_pack_u8', 'src', src)
    Hp, Wp = _pack_sides('resample_pack_u8', 'page_shape', page_shape)
    if out is not None and (tuple(out.shape) != (Hp, Wp, 3) or out.dtype != torch.uint8 or not out.is_contiguous()):
        raise ValueError(f'resample_pack_u8: out must be a contiguous {(Hp, Wp, 3)} uint8 tensor')
    table = _placements('resample_pack_u8', placements, (Hs, Ws), (Hp, Wp), src.device, validate)
    _require_cuda(src, out)
    if out is not None and out.device != src.device:
        raise ValueError(f'resample_pack_u8: out is on {out.device}, src on {src.device}')
    src = src.contiguous()
    page = out if out is not None else torch.empty((Hp, Wp, 3), dtype=torch.uint8, device=src.device)
    check(lib.vkas_resample_pack_u8(_p(src), Hs, Ws, _p(table) if table.shape[0] else None, int(table.shape[0]), _p(page),
                                    Hp, Wp, _stream()), 'resample_pack_u8')
    return page


def pack_region_labels(labels: torch.Tensor, valid_shape: Tuple[int, int], image_shape: Tuple[int, int], placements,
                       region_ids, out_shape: Tuple[int, int], fdf: int, validate: bool = True) -> torch.Tensor:
    """The int32 region-label page of a packed page at ``1/fdf`` of its resolution (csrc/respack.hip; the rule and the oracle:
    inferencing/packing.py::pack_region_labels_host).  labels (Hl,Wl) int32 on the device - the rough label map, of which
    ``valid_shape`` covers the ``image_shape`` image the placements' sources refer to; ``placements`` as in
    ``resample_pack_u8`` with the page taken as ``out_shape * fdf``; ``region_ids`` (n,) int32 >= 1, host or device.  Returns
    (Hq,Wq) int32: region_ids[k] where the pixel's centre lies in placement k and the rough map holds no other region's label
    at its source position, else 0."""
    Hl, Wl, vh, vw, Hs, Ws, Hq, Wq, fdf = _label_args('pack_region_labels', labels, valid_shape, image_shape, out_shape, fdf)
    table = _placements('pack_region_labels', placements, (Hs, Ws), (Hq * fdf, Wq * fdf), labels.device, validate)
    n = int(table.shape[0])
    ids = _region_ids('pack_region_labels', region_ids, n, labels.device)
    _require_cuda(labels)
    labels = labels.contiguous()
    out = torch.empty((Hq, Wq), dtype=torch.int32, device=labels.device)
    check(lib.vkas_pack_region_labels(_p(labels), Hl, Wl, vh, vw, Hs, Ws, _p(table) if n else None, _p(ids) if n else None, n,
                                      fdf, _p(out), Hq, Wq, _stream()), 'pack_region_labels')
    return out


def _multi_tables(who: str, sources, words: int, arena_size: int, rows, page_start, num_pages: int, page_shape, device,
                  validate: bool):
    """The three tables of a multi pack on ``device`` (each as ``_pack_table`` takes it): the (S, ``words``) int64 source
    table, the (n, 12) int32 rows and the (Q + 1,) int32 ``page_start`` (None: taken from the rows' page column).  What is
    checked on the host: every source entry inside the arena of ``arena_size`` elements, the rows by
    inferencing/packing.py::check_multi_rows, ``page_start`` against the rows."""
    import numpy as np
    from .inferencing.packing import check_multi_rows
    Q = int(num_pages)
    if Q != num_pages or not 1 <= Q <= 65535:
        raise ValueError(f'{who}: num_pages must be an integer in [1, 65535], got {num_pages}')
    d_sources, h_sources = _pack_table(who, 'sources', sources, (None, words), 'int64', device, validate)
    d_rows, h_rows = _pack_table(who, 'rows', rows, (None, 12), 'int32', device, validate)
    S, n = int(d_sources.shape[0]), int(d_rows.shape[0])
    if S < 1:
        raise ValueError(f'{who}: no sources')
    if h_sources is not None:
        t = h_sources
        if words == 4:  # (byte offset, Hs, Ws, 0): an (Hs, Ws, 3) uint8 image
            sides, need, shapes = t[:, 1:3], 3 * t[:, 1] * t[:, 2], t[:, 1:3]
        else:           # (word offset, Hl, Wl, valid_h, valid_w, Hs, Ws, 0): an (Hl, Wl) int32 map of an (Hs, Ws) image
            sides, need, shapes = t[:, [1, 2, 5, 6]], t[:, 1] * t[:, 2], t[:, 5:7]
            if ((t[:, 3] < 1) | (t[:, 3] > t[:, 1]) | (t[:, 4] < 1) | (t[:, 4] > t[:, 2])).any():
                raise ValueError(f'{who}: a valid part does not fit its label map')
        if ((sides < 1) | (sides > _PACK_DIM_MAX)).any():
            raise ValueError(f'{who}: source sides must be in [1, {_PACK_DIM_MAX}]')
        if ((t[:, 0] < 0) | (t[:, 0] + need > arena_size)).any():
            raise ValueError(f'{who}: a source leaves the arena of {arena_size} elements')
        if h_rows is not None:
            check_multi_rows(h_rows, shapes, page_shape, Q)
    elif h_rows is not None:
        raise ValueError(f'{who}: host rows need a host source table (or validate=True) to be checked against')
    if page_start is None:
        if h_rows is None:
            raise ValueError(f'{who}: page_start is needed with a device row table and validate=False')
        page_start = np.searchsorted(h_rows[:, 1], np.arange(Q + 1)).astype(np.int32)
    d_start, h_start = _pack_table(who, 'page_start', page_start, (Q + 1,), 'int32', device, validate)
    if h_start is not None:
        if h_rows is not None:
            if not np.array_equal(h_start, np.searchsorted(h_rows[:, 1], np.arange(Q + 1))):
                raise ValueError(f'{who}: page_start does not give each page its rows')
        elif h_start[0] < 0 or h_start[-1] > n or (np.diff(h_start) < 0).any():
            raise ValueError(f'{who}: page_start must rise from 0 to at most {n}')
    return d_sources, d_rows, d_start, S, n, Q


def resample_pack_u8_multi(arena: torch.Tensor, sources, rows, num_pages: int, page_shape: Tuple[int, int], page_start=None,
                           validate: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Crops, rescales and packs rectangles of several images into several pages in one launch (``infer_batch``;
    csrc/respack.hip).  ``arena``: a 1-D uint8 device tensor that holds the images; ``sources`` (S,4) int64 rows (byte
    offset, Hs, Ws, 0); ``rows`` (n,12) int32 multi rows (src, page, sy, sx, sh, sw, dy, dx, dh, dw, local_id, global_id)
    sorted by page; ``page_start`` (Q+1,) int32, computed from host rows when None - all three host or device (see
    ``_multi_tables``).  Returns the (Q,Hp,Wp,3) uint8 pages (``out`` if given), equal to
    inferencing/packing.py::resample_pack_multi_host byte for byte: every byte is written, zero where no row reaches.  With
    device tables and ``validate=False`` it never synchronises, so it can be captured into a HIP graph."""
    if arena.dim() != 1 or arena.dtype != torch.uint8:
        raise ValueError(f'resample_pack_u8_multi: arena must be a 1-D uint8 tensor, got {arena.dtype} {tuple(arena.shape)}')
    Hp, Wp = _pack_sides('resample_pack_u8_multi', 'page_shape', page_shape)
    if arena.numel() < 1 or not arena.is_contiguous():
        raise ValueError('resample_pack_u8_multi: arena must be contiguous and not empty')
    d_sources, d_rows, d_start, S, n, Q = _multi_tables('resample_pack_u8_multi', sources, 4, int(arena.numel()), rows,
                                                        page_start, num_pages, (Hp, Wp), arena.device, validate)
    if out is not None and (tuple(out.shape) != (Q, Hp, Wp, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or
                            out.device != arena.device):
        raise ValueError(f'resample_pack_u8_multi: out must be a contiguous {(Q, Hp, Wp, 3)} uint8 tensor on {arena.device}')
    _require_cuda(arena, out)
    pages = out if out is not None else torch.empty((Q, Hp, Wp, 3), dtype=torch.uint8, device=arena.device)
    check(lib.vkas_resample_pack_u8_multi(_p(arena), int(arena.numel()), _p(d_sources), S, _p(d_rows) if n else None, n,
                                          _p(d_start), _p(pages), Q, Hp, Wp, _stream()), 'resample_pack_u8_multi')
    return pages


def pack_region_labels_multi(label_arena: torch.Tensor, label_sources, rows, num_pages: int, out_shape: Tuple[int, int],
                             fdf: int, page_start=None, validate: bool = True,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The int32 label pages of ``resample_pack_u8_multi`` at ``1/fdf`` of the pages' resolution (csrc/respack.hip; the
    oracle: inferencing/packing.py::pack_region_labels_multi_host).  ``label_arena``: a 1-D int32 device tensor that holds
    the rough label maps of the batch; ``label_sources`` (S,8) int64 rows (word offset, Hl, Wl, valid_h, valid_w, Hs, Ws,
    0); ``rows`` / ``page_start`` as there, with the pages taken as ``out_shape * fdf``.  Returns (Q,Hq,Wq) int32 (``out`` if
    given): a row's ``global_id`` where the cell's centre lies in its destination and the rough map of its source holds
    neither another region's label than its ``local_id`` at the source position, else 0."""
    if label_arena.dim() != 1 or label_arena.dtype != torch.int32:
        raise ValueError(f'pack_region_labels_multi: label_arena must be a 1-D int32 tensor, got {label_arena.dtype} '
                         f'{tuple(label_arena.shape)}')
    fdf = _pack_factor('pack_region_labels_multi', fdf)
    Hq, Wq = _pack_sides('pack_region_labels_multi', 'label page', out_shape, fdf)
    if label_arena.numel() < 1 or not label_arena.is_contiguous():
        raise ValueError('pack_region_labels_multi: label_arena must be contiguous and not empty')
    d_sources, d_rows, d_start, S, n, Q = _multi_tables('pack_region_labels_multi', label_sources, 8, int(label_arena.numel()),
                                                        rows, page_start, num_pages, (Hq * fdf, Wq * fdf),
                                                        label_arena.device, validate)
    if out is not None and (tuple(out.shape) != (Q, Hq, Wq) or out.dtype != torch.int32 or not out.is_contiguous() or
                            out.device != label_arena.device):
        raise ValueError(f'pack_region_labels_multi: out must be a contiguous {(Q, Hq, Wq)} int32 tensor on {label_arena.device}')
    _require_cuda(label_arena, out)
    pages = out if out is not None else torch.empty((Q, Hq, Wq), dtype=torch.int32, device=label_arena.device)
    check(lib.vkas_pack_region_labels_multi(_p(label_arena), int(label_arena.numel()), _p(d_sources), S,
                                            _p(d_rows) if n else None, n, _p(d_start), fdf, _p(pages), Q, Hq, Wq, _stream()),
          'pack_region_labels_multi')
    return pages


def _label_maps(who: str, labels: torch.Tensor, max_regions) -> Tuple[int, int, int, int]:
    if labels.dim() != 3:
        raise ValueError(f'{who}: labels must be (B, H, W), got {tuple(labels.shape)}')
    if labels.dtype != torch.int32:
        raise ValueError(f'{who}: labels must be int32, got {labels.dtype}')
    B, H, W = (int(v) for v in labels.shape)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f'{who}: empty maps {(B, H, W)}')
    R = int(max_regions)
    if R != max_regions or R < 1:
        raise ValueError(f'{who}: max_regions must be an integer >= 1, got {max_regions}')
    if max(H, W) > _PACK_DIM_MAX or B > 65535:
        raise ValueError(f'{who}: map sides must not exceed {_PACK_DIM_MAX} and B 65535, got {(B, H, W)}')
    if B * H * W >= 1 << 31 or B * R >= 1 << 31:
        raise ValueError(f'{who}: B*H*W = {B * H * W} and B*R = {B * R} must stay below 2^31')
    return B, H, W, R


def region_moments(labels: torch.Tensor, max_regions: int) -> torch.Tensor:
    """The raw moments of the text regions (csrc/orient.hip; the oracle: inferencing/orient.py::region_moments_host).  labels
    (B,H,W) int32 on the device, as ``text_regions`` returns them.  Returns (B,R,6) int64 with R = ``max_regions``: row r-1 =
    ``n, sum y, sum x, sum y^2, sum x^2, sum x*y`` over the pixels of region r, exact; label 0 and labels above R are ignored,
    a region without pixels gets zeros.  Never synchronises, so it can be captured into a HIP graph."""
    B, H, W, R = _label_maps('region_moments', labels, max_regions)
    _require_cuda(labels)
    labels = labels.contiguous()
    out = torch.empty((B, R, 6), dtype=torch.int64, device=labels.device)
    check(lib.vkas_region_moments(_p(labels), B, H, W, R, _p(out), _stream()), 'region_moments')
    return out


_DIR_MAX = 1 << 14


def region_extents(labels: torch.Tensor, dirs, validate: bool = True) -> torch.Tensor:
    """The extents of the text regions along their own directions (csrc/orient.hip; the oracle: inferencing/orient.py::
    region_extents_host).  labels (B,H,W) int32 on the device; ``dirs`` (B,R,2) int32 ``(c, s)`` with ``|c|, |s| <= 2^14``,
    host (numpy / CPU tensor: always checked, then uploaded) or device (checked when ``validate`` - a synchronisation -, else
    trusted).  Returns (B,R,4) int32 ``min u, max u, min v, max v`` with ``u = c*x + s*y``, ``v = -s*x + c*y``; a region
    without pixels keeps ``(INT_MAX, INT_MIN, INT_MAX, INT_MIN)``."""
    import numpy as np
    if not isinstance(dirs, torch.Tensor):
        dirs = torch.from_numpy(np.ascontiguousarray(np.asarray(dirs)))
    if dirs.dim() != 3 or dirs.shape[2] != 2:
        raise ValueError(f'region_extents: dirs must be (B, R, 2), got {tuple(dirs.shape)}')
    if dirs.dtype != torch.int32:
        raise ValueError(f'region_extents: dirs must be int32, got {dirs.dtype}')
    B, H, W, R = _label_maps('region_extents', labels, int(dirs.shape[1]))
    if dirs.shape[0] != B:
        raise ValueError(f'region_extents: dirs must be ({B}, R, 2), got {tuple(dirs.shape)}')
    if (validate or not dirs.is_cuda) and int(dirs.abs().max()) > _DIR_MAX:
        raise ValueError(f'region_extents: |c| and |s| must not exceed {_DIR_MAX}')
    _require_cuda(labels)
    if dirs.is_cuda and dirs.device != labels.device:
        raise ValueError(f'region_extents: dirs are on {dirs.device}, labels on {labels.device}')
    dirs = dirs.to(labels.device, non_blocking=True).contiguous()
    labels = labels.contiguous()
    out = torch.empty((B, R, 4), dtype=torch.int32, device=labels.device)
    check(lib.vkas_region_extents(_p(labels), B, H, W, R, _p(dirs), _p(out), _stream()), 'region_extents')
    return out


def warp_pack_u8(src: torch.Tensor, warps, page: torch.Tensor, validate: bool = True) -> torch.Tensor:
    """Cuts slanted rectangles out of one image along their own axes into a page (csrc/respack.hip; the rule and the oracle:
    inferencing/packing.py::warp_host).  src (Hs,Ws,3) uint8 and ``page`` (Hp,Wp,3) uint8, contiguous, on the device;
    ``warps`` (K,12) int64 rows, host or device (as ``resample_pack_u8`` takes placements).  Writes ONLY the pixels inside
    the warps' destinations - it runs after ``resample_pack_u8`` has written the page and its zeros - and returns ``page``.
    The destinations must also be disjoint from that call's placements (``check_warps(..., placements)``: the caller's
    check).  One launch; with a device table and ``validate=False`` it never synchronises."""
    Hs, Ws = _pack_image('warp_pack_u8', 'src', src)
    Hp, Wp = _pack_image('warp_pack_u8', 'page', page)
    if not page.is_contiguous():
        raise ValueError('warp_pack_u8: page must be contiguous (it is written in place)')
    table = _warps('warp_pack_u8', warps, (Hp, Wp), src.device, validate)
    _require_cuda(src, page)
    if page.device != src.device:
        raise ValueError(f'warp_pack_u8: page is on {page.device}, src on {src.device}')
    src = src.contiguous()
    K = int(table.shape[0])
    check(lib.vkas_warp_pack_u8(_p(src), Hs, Ws, _p(table) if K else None, K, _p(page), Hp, Wp, _stream()), 'warp_pack_u8')
    return page


def warp_region_labels(labels: torch.Tensor, valid_shape: Tuple[int, int], image_shape: Tuple[int, int], warps, region_ids,
                       out: torch.Tensor, fdf: int, validate: bool = True) -> torch.Tensor:
    """The label cells of the warps, written into the (Hq,Wq) int32 label page ``out`` of ``pack_region_labels`` (csrc/
    respack.hip; the rule and the oracle: inferencing/packing.py::warp_region_labels_host).  Arguments as
    ``pack_region_labels`` with ``warps`` as in ``warp_pack_u8``; writes ONLY the cells whose centres lie inside the warps'
    destinations and returns ``out``."""
    if out.dim() != 2 or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f'warp_region_labels: out must be a contiguous (H, W) int32 tensor (it is written in place), got '
                         f'{out.dtype} {tuple(out.shape)}')
    Hl, Wl, vh, vw, Hs, Ws, Hq, Wq, fdf = _label_args('warp_region_labels', labels, valid_shape, image_shape, out.shape,
                                                      fdf)
    table = _warps('warp_region_labels', warps, (Hq * fdf, Wq * fdf), labels.device, validate)
    K = int(table.shape[0])
    ids = _region_ids('warp_region_labels', region_ids, K, labels.device)
    _require_cuda(labels, out)
    if out.device != labels.device:
        raise ValueError(f'warp_region_labels: out is on {out.device}, labels on {labels.device}')
    labels = labels.contiguous()
    check(lib.vkas_warp_region_labels(_p(labels), Hl, Wl, vh, vw, Hs, Ws, _p(table) if K else None, _p(ids) if K else None, K,
                                      fdf, _p(out), Hq, Wq, _stream()), 'warp_region_labels')
    return out


_CROP_SIDE_MAX = 8192


def image_arena(mats, device):
    """(H, W, 3) uint8 arrays in ONE device byte arena: copied once into one pinned host buffer, every image start 16-byte
    aligned, and uploaded in one transfer.  -> the arena (1-D uint8 on ``device``) and its (S, 4) int64 source table (byte
    offset, Hs, Ws, 0) on the host and on the device - what ``resample_pack_u8_multi`` and ``crop_warp`` read."""
    import numpy as np
    table = np.zeros((len(mats), 4), np.int64)
    total = 0
    for i, m in enumerate(mats):
        if m.dtype != np.uint8:
            raise ValueError(f'image {i}: a batch takes uint8 images, got {m.dtype}')
        if min(m.shape[:2]) < 1 or max(m.shape[:2]) > _CROP_SIDE_MAX:
            raise ValueError(f'image {i} {m.shape[:2]}: the device resampler takes sides from 1 to {_CROP_SIDE_MAX}')
        table[i] = (total, m.shape[0], m.shape[1], 0)
        total += -(-m.size // 16) * 16
    host = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    flat = host.numpy()
    for m, (offset, _, _, _) in zip(mats, table.tolist()):
        flat[offset:offset + m.size] = m.reshape(-1)
    return host.to(device, non_blocking=True), table, torch.from_numpy(table).to(device, non_blocking=True)


def _strip_height(who: str, h) -> int:
    from .inferencing.strips import HEIGHT_MAX
    if h != int(h) or not 1 <= int(h) <= HEIGHT_MAX:
        raise ValueError(f'{who}: h must be an integer in [1, {HEIGHT_MAX}], got {h}')
    return int(h)


def _strip_args(who: str, arena: torch.Tensor, sources, h, out_bytes, validate: bool):
    """What the strip ops take alike, checked: the arena, the height, the output size and the source table (as ``_pack_table``
    takes tables) -> ``(h, out_bytes, device sources, host sources or None)``."""
    if arena.dim() != 1 or arena.dtype != torch.uint8:
        raise ValueError(f'{who}: arena must be a 1-D uint8 tensor, got {arena.dtype} {tuple(arena.shape)}')
    if arena.numel() < 1 or not arena.is_contiguous():
        raise ValueError(f'{who}: arena must be contiguous and not empty')
    h, out_bytes = _strip_height(who, h), int(out_bytes)
    if not 0 <= out_bytes < 1 << 40:
        raise ValueError(f'{who}: out_bytes must be in [0, 2^40), got {out_bytes}')
    d_sources, h_sources = _pack_table(who, 'sources', sources, (None, 4), 'int64', arena.device, validate)
    if int(d_sources.shape[0]) < 1:
        raise ValueError(f'{who}: no sources')
    return h, out_bytes, d_sources, h_sources


def _strip_host_sources(who: str, need: str, arena: torch.Tensor, h_sources) -> None:
    """Before host rows are checked against their sources: these are on the host as well and stay inside the arena."""
    if h_sources is None:
        raise ValueError(f'{who}: {need} a host source table (or validate=True) to be checked against')
    if ((h_sources[:, 0] < 0) | (h_sources[:, 0] + 3 * h_sources[:, 1] * h_sources[:, 2] > int(arena.numel()))).any():
        raise ValueError(f'{who}: a source leaves the arena of {int(arena.numel())} bytes')


def quad_strips_u8(arena: torch.Tensor, sources, rows, h: int, out_bytes: int, validate: bool = True) -> torch.Tensor:
    """Cuts text lines out of the images of an arena into upright strips of height ``h``, all in one launch (csrc/strips.hip;
    the rule, the row layout and the oracle: inferencing/strips.py).  ``arena``: a 1-D uint8 device tensor that holds the
    images; ``sources`` (S,4) int64 rows (byte offset, Hs, Ws, 0) as ``image_arena`` builds them; ``rows``: the (n,12) int64
    strip rows, host or device, or the 1-D int64 device table ``strips.strip_table`` lays out (the rows, then ``tile_start``)
    - from (n,12) rows that table is built here, on the host for host rows, with a few small device operations for device
    rows.  Host tables are always checked (``check_strip_rows``), device tables when ``validate`` - a synchronisation.
    Returns the 1-D uint8 output of ``out_bytes`` bytes: every byte of every slot is written - the slots of ``strip_rows``
    cover the output -, a byte outside the slots keeps what the allocation held.  Allocates only its output (and the small
    table); with device tables and ``validate=False`` it never synchronises, so it can be captured into a HIP graph."""
    import numpy as np
    from .inferencing.strips import ROW_WORDS, TILE_H, TILE_W, check_strip_rows, strip_table
    h, out_bytes, d_sources, h_sources = _strip_args('quad_strips_u8', arena, sources, h, out_bytes, validate)
    flat = isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 1
    if flat:
        if (int(rows.numel()) - 1) % (ROW_WORDS + 1):
            raise ValueError(f'quad_strips_u8: a 1-D row table holds 13*n + 1 words, got {int(rows.numel())}')
        d_table, h_table = _pack_table('quad_strips_u8', 'rows', rows, (None,), 'int64', arena.device, validate)
        n = (int(d_table.numel()) - 1) // (ROW_WORDS + 1)
        h_rows = None if h_table is None else h_table[:n * ROW_WORDS].reshape(n, ROW_WORDS)
        if h_table is not None and not np.array_equal(h_table, strip_table(h_rows, h)):
            raise ValueError('quad_strips_u8: tile_start does not give each row its tiles')
    else:
        d_rows, h_rows = _pack_table('quad_strips_u8', 'rows', rows, (None, ROW_WORDS), 'int64', arena.device, validate)
        n = int(d_rows.shape[0])
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            tiles = -(-h // TILE_H) * ((d_rows[:, 2].clamp(0, 8192) + (TILE_W - 1)) // TILE_W)
            d_table = torch.cat([d_rows.reshape(-1), tiles.new_zeros(1), tiles.cumsum(0)])
        else:
            d_table = torch.from_numpy(strip_table(h_rows, h)).to(arena.device, non_blocking=True)
    if h_rows is not None:
        _strip_host_sources('quad_strips_u8', 'host rows need', arena, h_sources)
        check_strip_rows(h_rows, h_sources, h, out_bytes)
    _require_cuda(arena)
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=arena.device)
    if n:
        check(lib.vkas_quad_strips_u8(_p(arena), int(arena.numel()), _p(d_sources), int(d_sources.shape[0]), _p(d_table), n, h,
                                      _p(out), out_bytes, _stream()), 'quad_strips_u8')
    return out


def _spine_table(who: str, table, n: int, knots_total: int, h: int, device, validate: bool):
    """The 1-D int64 table of ``spines.spine_table`` (host or device, as ``_pack_table`` takes tables) on the device, and its
    host rows and knots (None for a trusted device table).  ``h`` is checked (``_strip_height``)."""
    import numpy as np
    from .inferencing.spines import KNOT_WORDS, spine_table
    from .inferencing.strips import ROW_WORDS
    n, knots_total = int(n), int(knots_total)
    if n < 0 or knots_total < 0:
        raise ValueError(f'{who}: n and knots_total must be at or above 0, got {n}, {knots_total}')
    d_table, h_table = _pack_table(who, 'table', table, (None,), 'int64', device, validate)
    words = (ROW_WORDS + 1) * n + 1 + KNOT_WORDS * knots_total
    if int(d_table.numel()) != words:
        raise ValueError(f'{who}: a table of {n} rows and {knots_total} knots holds {words} words, got {int(d_table.numel())}')
    if h_table is None:
        return d_table, None, None
    h_rows = h_table[:n * ROW_WORDS].reshape(n, ROW_WORDS)
    h_knots = h_table[(ROW_WORDS + 1) * n + 1:].reshape(knots_total, KNOT_WORDS)
    if not np.array_equal(h_table, spine_table(h_rows, h_knots, h)):
        raise ValueError(f'{who}: tile_start does not give each row its tiles')
    return d_table, h_rows, h_knots


def spine_columns(table, n: int, knots_total: int, h: int, columns: int, validate: bool = True) -> torch.Tensor:
    """The column records of the spine rows of a table (``spines.spine_table``), as the first launch of ``spine_strips_u8``
    writes them: a (columns, 6) int64 device tensor, row r's records at ``col_start .. col_start + w - 1``, every record no
    row owns ``INT64_MIN``.  Equal to ``spines.spine_columns_host`` word for word.  For the tests."""
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        raise ValueError('spine_columns: table must be a device tensor')
    h = _strip_height('spine_columns', h)
    d_table, h_rows, h_knots = _spine_table('spine_columns', table, n, knots_total, h, table.device, validate)
    n, columns = int(n), int(columns)
    if not n <= columns < 1 << 40:
        raise ValueError(f'spine_columns: columns must be in [n, 2^40), got {columns}')
    if h_rows is not None and len(h_rows) and (h_rows[:, 6].min() < 0 or (h_rows[:, 6] + h_rows[:, 3]).max() > columns):
        raise ValueError(f'spine_columns: a row\'s columns leave the {columns} records')
    out = torch.full((columns, 6), -(1 << 63), dtype=torch.int64, device=d_table.device)
    if n:
        check(lib.vkas_spine_columns(_p(d_table), n, int(knots_total), h, _p(out), columns, _stream()), 'spine_columns')
    return out


def spine_strips_u8(arena: torch.Tensor, sources, table, n: int, knots_total: int, h: int, out_bytes: int,
                    validate: bool = True) -> torch.Tensor:
    """Cuts curved text lines out of the images of an arena into strips of height ``h`` along their spines, two launches on
    one stream (csrc/spines.hip; the rule, the table layout and the oracle: inferencing/spines.py).  ``arena`` and ``sources``
    as in ``quad_strips_u8``; ``table``: the 1-D int64 table ``spines.spine_table`` lays out - ``n`` spine rows, ``tile_start``,
    ``knots_total`` knot records.  Host tables are always checked (``check_spine_rows``), device tables when ``validate`` - a
    synchronisation.  Returns the 1-D uint8 output of ``out_bytes`` bytes: every byte of every slot is written, a byte outside
    the slots keeps what the allocation held.  Allocates only its output and the workspace of the column records -
    ``out_bytes // (3*h)`` of them, which disjoint slots inside the output cannot exceed -; with device tables and
    ``validate=False`` it never synchronises, so it can be captured into a HIP graph."""
    from .inferencing.spines import check_spine_rows
    h, out_bytes, d_sources, h_sources = _strip_args('spine_strips_u8', arena, sources, h, out_bytes, validate)
    d_table, h_rows, h_knots = _spine_table('spine_strips_u8', table, n, knots_total, h, arena.device, validate)
    n, knots_total = int(n), int(knots_total)
    columns = out_bytes // (3 * h)
    if h_rows is not None:
        _strip_host_sources('spine_strips_u8', 'a host table needs', arena, h_sources)
        check_spine_rows(h_rows, h_knots, h_sources, h, out_bytes, columns)
    if columns < n:
        raise ValueError(f'spine_strips_u8: an output of {out_bytes} bytes has no room for the slots of {n} rows')
    _require_cuda(arena)
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=arena.device)
    if n:
        ws = torch.empty((max(columns, 1) * 6,), dtype=torch.int64, device=arena.device)
        check(lib.vkas_spine_strips_u8(_p(arena), int(arena.numel()), _p(d_sources), int(d_sources.shape[0]), _p(d_table), n,
                                       knots_total, h, _p(ws), int(ws.numel()) * 8, _p(out), out_bytes, _stream()),
              'spine_strips_u8')
    return out


def _crop_warp_args(who: str, arena: torch.Tensor, sources, rows, size, validate: bool, out):
    """What the crop ops take alike, checked before anything is launched -> ``(device sources, device rows, host rows or None,
    S, B, H, W)``."""
    import numpy as np
    from .dataset.crops import check_crop_rows
    if arena.dim() != 1 or arena.dtype != torch.uint8:
        raise ValueError(f'{who}: arena must be a 1-D uint8 tensor, got {arena.dtype} {tuple(arena.shape)}')
    if arena.numel() < 1 or not arena.is_contiguous():
        raise ValueError(f'{who}: arena must be contiguous and not empty')
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: size must be (height, width), got {size!r}') from None
    if not (1 <= H <= _CROP_SIDE_MAX and 1 <= W <= _CROP_SIDE_MAX):
        raise ValueError(f'{who}: size sides must be in [1, {_CROP_SIDE_MAX}], got {(H, W)}')
    d_sources, h_sources = _pack_table(who, 'sources', sources, (None, 4), 'int64', arena.device, validate)
    d_rows, h_rows = _pack_table(who, 'rows', rows, (None, 16), 'int64', arena.device, validate)
    S, B = int(d_sources.shape[0]), int(d_rows.shape[0])
    if S < 1:
        raise ValueError(f'{who}: no sources')
    if B > 65535:
        raise ValueError(f'{who}: B = {B} above 65535')
    if h_sources is not None:
        t = h_sources
        if ((t[:, 1:3] < 1) | (t[:, 1:3] > _CROP_SIDE_MAX)).any():
            raise ValueError(f'{who}: source sides must be in [1, {_CROP_SIDE_MAX}]')
        if ((t[:, 0] < 0) | (t[:, 0] + 3 * t[:, 1] * t[:, 2] > int(arena.numel()))).any():
            raise ValueError(f'{who}: a source leaves the arena of {int(arena.numel())} bytes')
        if h_rows is not None:
            check_crop_rows(h_rows, t[:, 1:3])
    elif h_rows is not None:
        raise ValueError(f'{who}: host rows need a host source table (or validate=True) to be checked against')
    if out is not None and (tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or
                            out.device != arena.device):
        raise ValueError(f'{who}: out must be a contiguous {(B, 3, H, W)} float32 tensor on {arena.device}')
    return d_sources, d_rows, h_rows, S, B, H, W


def crop_warp(arena: torch.Tensor, sources, rows, size: Tuple[int, int], validate: bool = True,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Training crops of annotated pages: one affine map and one photometric jitter per output image, in one launch
    (csrc/crops.hip; the rule and the oracle: dataset/crops.py::crop_host).  ``arena``: a 1-D uint8 device tensor that holds
    the pages; ``sources`` (S,4) int64 rows (byte offset, Hs, Ws, 0) as ``image_arena`` builds them; ``rows`` (B,16) int64
    crop rows - both host or device (as ``_pack_table`` takes them: host tables are always checked, device tables when
    ``validate``, a synchronisation).  Returns the (B,3,H,W) float32 crops (``out`` if given), equal to ``crop_host`` bit for
    bit: every element is written.  An unchecked row that cannot be trusted gives a zero image (see include/vkas.h).
    Allocates only its output; with device tables and ``validate=False`` it never synchronises, so it can be captured into a
    HIP graph."""
    d_sources, d_rows, _, S, B, H, W = _crop_warp_args('crop_warp', arena, sources, rows, size, validate, out)
    _require_cuda(arena, out)
    crops = out if out is not None else torch.empty((B, 3, H, W), dtype=torch.float32, device=arena.device)
    if B:
        check(lib.vkas_crop_warp_f32(_p(arena), int(arena.numel()), _p(d_sources), S, _p(d_rows), B, _p(crops), H, W,
                                     _stream()), 'crop_warp')
    return crops


_BLUR_RADIUS_MAX = 7


def crop_blur_work_bytes(B: int, size: Tuple[int, int], radius_max: int = _BLUR_RADIUS_MAX) -> int:
    """The bytes of ``crop_warp_blur``'s ``work``: uint8 planes (B, 3, H + 2*radius_max, pitch), the pitch a multiple of 16."""
    H, W = (int(v) for v in size)
    return int(B) * 3 * (H + 2 * radius_max) * (-(-(W + 2 * radius_max) // 16) * 16)


def crop_warp_blur(arena: torch.Tensor, sources, rows, blur_rows, size: Tuple[int, int], validate: bool = True,
                   out: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None,
                   radius_max: Optional[int] = None) -> torch.Tensor:
    """``crop_warp`` with one blur table per output image between the geometric value and the jitter, in two launches
    (csrc/crops.hip; the rule and the oracle: dataset/blur.py::crop_blur_host).  ``arena``, ``sources``, ``rows``, ``size`` and
    ``out`` as in ``crop_warp``; ``blur_rows`` (B,226) int32, host or device, checked like the rows (``check_blur_rows``).
    ``radius_max`` in [0, 7] bounds the radii and sizes the halo of the intermediate: by default the table's maximum for a
    table that is on the host and 7 otherwise; an unchecked row above it gives a zero image, as an invalid one does.
    ``work``: a 1-D uint8 device tensor of at least ``crop_blur_work_bytes(B, size, radius_max)`` bytes, 16-byte aligned,
    allocated when not given.  Returns the (B,3,H,W) float32 crops, equal to ``crop_blur_host`` bit for bit.  With host tables
    whose radii are all 0 it is ``crop_warp`` and nothing else.  With device tables, ``validate=False`` and ``work`` and
    ``out`` given it neither allocates nor synchronises, so it can be captured into a HIP graph."""
    from .dataset.blur import check_blur_rows
    d_sources, d_rows, _, S, B, H, W = _crop_warp_args('crop_warp_blur', arena, sources, rows, size, validate, out)
    on_host = not (isinstance(blur_rows, torch.Tensor) and blur_rows.is_cuda)
    d_blur, h_blur = _pack_table('crop_warp_blur', 'blur_rows', blur_rows, (B, 226), 'int32', arena.device, validate,
                                 check_blur_rows)
    table_max = int(h_blur[:, 0].max()) if h_blur is not None and B else 0
    if radius_max is None:
        radius_max = table_max if on_host else _BLUR_RADIUS_MAX
    if radius_max != int(radius_max) or not 0 <= int(radius_max) <= _BLUR_RADIUS_MAX:
        raise ValueError(f'crop_warp_blur: radius_max must be an integer in [0, {_BLUR_RADIUS_MAX}], got {radius_max}')
    radius_max = int(radius_max)
    if h_blur is not None and table_max > radius_max:
        raise ValueError(f'crop_warp_blur: a blur row has radius {table_max}, above radius_max = {radius_max}')
    need = crop_blur_work_bytes(B, (H, W), radius_max)
    if work is not None and (work.dim() != 1 or work.dtype != torch.uint8 or not work.is_contiguous() or
                             work.device != arena.device or int(work.numel()) < need or work.data_ptr() % 16):
        raise ValueError(f'crop_warp_blur: work must be a contiguous 16-byte aligned 1-D uint8 tensor of at least {need} bytes '
                         f'on {arena.device}')
    if on_host and table_max == 0:
        return crop_warp(arena, d_sources, d_rows, (H, W), validate=False, out=out)  # the tables are checked and uploaded
    _require_cuda(arena, out)
    crops = out if out is not None else torch.empty((B, 3, H, W), dtype=torch.float32, device=arena.device)
    if B:
        if work is None:
            work = torch.empty((need,), dtype=torch.uint8, device=arena.device)
        check(lib.vkas_crop_warp_blur_f32(_p(arena), int(arena.numel()), _p(d_sources), S, _p(d_rows), _p(d_blur), B, radius_max,
                                          _p(work), int(work.numel()), _p(crops), H, W, _stream()), 'crop_warp_blur')
    return crops
