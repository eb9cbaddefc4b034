"""Convolution with HIP kernels in all three directions (forward, input gradient, weight gradient) as a torch.autograd
Function.  Replaces nn.Conv2d's forward AND backward on the training path (reference: every nn.Conv2d of
CVSR_train/arch/CVSR_freq.py under `loss.backward()`, train_LD_freqCVSR_S_22.py:244-251).

Tensors are (B,C,H,W) in torch's channels_last memory format, i.e. NHWC in memory, the layout of the HIP kernels: the
(B,H,W,C) permutation handed to the C ABI is a zero-copy view.

precision "f32": exact-f32 kernels in all directions (the mode the gradient goldens are checked in).
precision "bf16"/"f16": forward and input gradient on the matrix cores (fcvsr_conv2d_mfma, f32 accumulate) when the layer is
eligible (1x1 / 3x3, channel counts the MFMA path takes); weight gradient with bf16 products on the matrix cores for the
3x3 / 1x1 layers with multiples of 64 channels (fcvsr_conv2d_wgrad_mfma), exact f32 for the rest.

Round 3: a layer is ONE forward launch and at most five backward launches.  Bias and LeakyReLU / ReLU ride in the forward
kernel's epilogue (`act`, `slope`); the activation's backward is one elementwise launch on the saved OUTPUT; the bias gradient is
a two-stage column sum, or a by-product of the matrix-core weight gradient; the 16-bit operand packings of the weight (forward and
transposed + tap-flipped for the input gradient) are one launch for all weights of a training pass (WeightPacker) - they were
chains of 4-8 small torch kernels per layer and step.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from typing import Dict, List, Optional, Tuple

import torch

from .. import hip

_MMA = {"bf16": (hip.BF16, torch.bfloat16), "f16": (hip.F16, torch.float16)}
_ACT = {None: hip.ACT_NONE, "none": hip.ACT_NONE, "relu": hip.ACT_RELU, "lrelu": hip.ACT_LEAKY}

# Storages (device, pointer) of the flat gradient buffers of the accumulate_into_grad contexts open right now.  Not thread-local: the
# autograd backward runs on a worker thread; the storage test in _grad_sink is what keeps other backwards out.
_ACTIVE = []


@contextlib.contextmanager
def accumulate_into_grad(*buffers: torch.Tensor):
    """While open (TrainStep wraps loss.backward() with its flat gradient buffer), the weight / bias gradient of a parameter whose
    `.grad` is a dense f32 view of one of `buffers` is ADDED into that `.grad` by the reduction kernel itself and the autograd
    Function returns None for it: no AccumulateGrad addition per parameter and pass (and no gradient hooks for those parameters).
    Parameters whose `.grad` lies anywhere else (another model, no `.grad` yet) and every backward outside the context get ordinary
    gradients."""
    keys = [(b.device, b.untyped_storage().data_ptr()) for b in buffers]
    _ACTIVE.extend(keys)
    try:
        yield
    finally:
        for k in keys:
            _ACTIVE.remove(k)


def _grad_sink(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The parameter's `.grad` if the reductions may add into it in place, else None."""
    if not _ACTIVE or p is None or not p.is_leaf:
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
        return None
    return g if (g.device, g.untyped_storage().data_ptr()) in _ACTIVE else None


def grad_destinations(*params: torch.Tensor) -> Tuple[List[torch.Tensor], int, List[Optional[torch.Tensor]]]:
    """Where ONE backward kernel puts the gradients of `params`: (destinations, accumulate flag of the kernel, what the autograd
    Function returns for them).  Either every parameter's `.grad` is a sink (accumulate = 1, autograd gets None) or none is used
    (fresh f32 tensors in the parameters' shapes, accumulate = 0, autograd gets them)."""
    sinks = [_grad_sink(p) for p in params]
    if all(g is not None for g in sinks):
        return sinks, 1, [None] * len(params)
    fresh = [torch.empty(p.shape, dtype=torch.float32, device=p.device) for p in params]
    return fresh, 0, fresh


def pack_weight_mfma(w: torch.Tensor, tdt: torch.dtype, transposed: bool) -> torch.Tensor:
    """16-bit operand layout of fcvsr_conv2d_mfma for `w` (or for the input-gradient convolution), one HIP launch."""
    cout, cin, kh, kw = w.shape
    rows, cols = (cin, cout) if transposed else (cout, cin)
    rp, cp = (rows + 127) // 128 * 128, (cols + 63) // 64 * 64
    out = torch.empty((kh * kw, rp, cp), dtype=tdt, device=w.device)
    wd = w.detach()
    if wd.dtype != torch.float32 or not wd.is_contiguous():
        wd = wd.float().contiguous()
    hip.check(hip.lib().fcvsr_pack_weight_mfma(wd.data_ptr(), cout, cin, kh, kw, out.data_ptr(), rp, cp, hip._DT[tdt], int(transposed),
                                               hip.stream_ptr()), "fcvsr_pack_weight_mfma")
    return out


class WeightPacker:
    """The 16-bit weight operands of ONE parameter set's training passes (a model at one train precision, see
    _GShiftBase.train_packer).  Within a pass a packing is cached per (storage pointer, parameter version, dtype, transposed), so a
    layer applied several times packs once; across passes nothing is reused, because the optimizer rewrites every weight.  The
    packings a pass asked for (leaf parameters only: their storage is stable) are recorded and, from the next pass on, replayed as
    ONE launch at the start of the pass (fcvsr_pack_weights_mfma_multi) from a device table: the plan.  A hipGraph that captured
    a pass records raw pointers into the plan's table and packed tensors, so its owner keeps the plan object alive
    (TrainStep._graphed)."""

    def __init__(self, model=None):
        self.owner = weakref.ref(model) if model is not None else None     # the model that holds this packer (its deepcopy guard)
        self.plan = None            # dict(items=[(weight, dtype, transposed, packed)], tabs={dtype: (table, n_items, blocks)}, ...)
        self._record = []           # requests of the pass in progress (while no plan exists)
        self._packed: Dict[Tuple, torch.Tensor] = {}

    @staticmethod
    def _key(w, tdt, transposed):
        return (w.data_ptr(), w._version, tdt, transposed, tuple(w.shape), str(w.device))

    def begin_pass(self) -> None:
        """Start of a differentiable pass (graph.forward_train): forget the cached packings; when the previous passes left a plan
        (same storage), re-pack all of its weights from their current values in one launch.  Also guarantees that a hipGraph
        capture records the packing kernels of its pass."""
        self._packed.clear()
        if self.plan is None and self._record and not torch.cuda.is_current_stream_capturing():
            self.plan = _build_plan(self._record)            # (uploads the table: never inside a capture)
        self._record = []
        if self.plan is None:
            return
        items = self.plan["items"]
        if any(w.data_ptr() != ptr or w.dtype != torch.float32 or not w.is_contiguous() or w.device != self.plan["device"]
               for (w, _, _, _), ptr in zip(items, self.plan["ptrs"])):
            self.plan = None                                 # parameters moved: record again during this pass
            return
        L = hip.lib()
        for tdt, (tab, n, blocks) in self.plan["tabs"].items():
            hip.check(L.fcvsr_pack_weights_mfma_multi(tab.data_ptr(), n, blocks, hip._DT[tdt], hip.stream_ptr()), "fcvsr_pack_weights_mfma_multi")
        for (w, tdt, transposed, out) in items:
            self._packed[self._key(w, tdt, transposed)] = out

    def get(self, w: torch.Tensor, tdt: torch.dtype, transposed: bool) -> torch.Tensor:
        """pack_weight_mfma(w, tdt, transposed), cached for the pass in progress."""
        key = self._key(w, tdt, transposed)
        out = self._packed.get(key)
        if out is None:
            out = self._packed[key] = pack_weight_mfma(w, tdt, transposed)
            if self.plan is None and w.is_leaf and w.dtype == torch.float32 and w.is_contiguous():
                self._record.append((w, tdt, transposed, out))   # a parameter in stable storage: part of the next passes' one launch
        return out


def _packed(packer: Optional[WeightPacker], w: torch.Tensor, tdt: torch.dtype, transposed: bool) -> torch.Tensor:
    return packer.get(w, tdt, transposed) if packer is not None else pack_weight_mfma(w, tdt, transposed)


def _build_plan(items):
    dev = items[0][0].device
    be = hip.lib().fcvsr_pack_weights_multi_block_elems()
    tabs = {}
    for tdt in set(it[1] for it in items):
        rows, blk = [], 0
        for (w, t, transposed, out) in items:
            if t != tdt:
                continue
            cout, cin, kh, kw = w.shape
            kk, rp, cp = out.shape
            rows.append([w.data_ptr(), out.data_ptr(), cout, cin, kk, rp, cp, int(transposed), blk])
            blk += (kk * rp * cp + be - 1) // be
        tabs[tdt] = (torch.tensor(rows, dtype=torch.int64).to(dev), len(rows), blk)
    return dict(items=items, tabs=tabs, device=dev, ptrs=[it[0].data_ptr() for it in items])


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """(B,C,H,W) any layout -> contiguous (B,H,W,C) view of a channels_last tensor, with the dense strides."""
    v = t.permute(0, 2, 3, 1).contiguous()               # no copy when t is already channels_last
    # contiguous() keeps any stride of a size-1 dimension (an NCHW (B, C, 1, 1) gradient stays (C, 1, 1, 1)), which the kernels' stride
    # alignment checks reject: restate the dense ones (same elements, no copy)
    _, H, W, Cn = v.shape
    dense = (H * W * Cn, W * Cn, Cn, 1)
    return v if v.stride() == dense else v.as_strided(v.shape, dense)


def _run_conv(x_nhwc: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, precision: str,
              packer: Optional[WeightPacker], *, transposed: bool = False, act: int = hip.ACT_NONE, slope: float = 0.0) -> torch.Tensor:
    """x (B,H,W,Cin) f32, w (Cout,Cin,k,k) [transposed: the input-gradient convolution with w^T, taps flipped] -> (B,Ho,Wo,Cout) f32
    ("same" padding k//2), bias and activation in the kernel's epilogue."""
    cout, cin, k, _ = w.shape
    if transposed:
        cout, cin = cin, cout
    B, H, W, _ = x_nhwc.shape
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=x_nhwc.device)
    b = None if bias is None else bias.detach()
    if b is not None and (b.dtype != torch.float32 or not b.is_contiguous()):
        b = b.float().contiguous()
    if precision in _MMA and k in (1, 3) and stride == 1 and cin % 4 == 0 and (cout % 4 == 0 or cout < 4):
        mdt, tdt = _MMA[precision]
        co4, dst, b4 = cout, out, b
        if cout < 4:             # conv_last0 (64 -> 1 at 4H x 4W): run as a 4-channel layer, the packed weight rows past cout are zero
            co4 = 4
            dst = torch.empty((B, Ho, Wo, 4), dtype=torch.float32, device=x_nhwc.device)
            b4 = None if b is None else torch.nn.functional.pad(b, (0, 4 - cout))
        groups = [dict(srcs=[x_nhwc], dst=dst)]
        if hip.mfma_eligible(k, stride, groups):
            hip.conv2d_mfma(groups, _packed(packer, w, tdt, transposed), k, co4, mdt, bias=b4, act=act, slope=slope)
            return dst if co4 == cout else dst[..., :cout]
    wl = w.detach()
    if transposed:
        wl = wl.permute(1, 0, 2, 3).flip(2, 3).contiguous()
    wm = hip.pack_conv_weight_f32mfma(wl) if (k in (1, 3) and stride == 1 and cin % 32 == 0 and cout % 4 == 0) else None
    hip.conv2d([x_nhwc], hip.pack_conv_weight(wl), k, cout, out, bias=b, stride=stride, w_f32mfma=wm, act=act, slope=slope)
    return out


def _colsum(g_nhwc: torch.Tensor, out: torch.Tensor, accumulate: int) -> None:
    """out (=, or += with accumulate) sum over (b, y, x) of a dense (B,H,W,C) f32 tensor: the bias gradient."""
    Cn = g_nhwc.shape[3]
    npix = g_nhwc.numel() // Cn
    L = hip.lib()
    n = L.fcvsr_colsum_scratch_elems(npix, Cn)
    scratch = torch.empty(n, dtype=torch.float32, device=g_nhwc.device)
    hip.check(L.fcvsr_colsum(g_nhwc.data_ptr(), npix, Cn, out.data_ptr(), scratch.data_ptr(), n, accumulate, hip.stream_ptr()), "fcvsr_colsum")


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, precision, act, slope, packer):
        xv = _nhwc(x.float())
        out = _run_conv(xv, w, bias, stride, precision, packer, act=act, slope=slope)
        # the activation backward reads the saved output as a dense (npix, cout) array: 1-3 output channels in a 16-bit mode come back as
        # a strided view of a 4-channel buffer, which is compacted here
        ctx.save_for_backward(xv, w, out.contiguous() if act != hip.ACT_NONE else None, bias)
        ctx.stride, ctx.precision, ctx.has_bias, ctx.act, ctx.slope, ctx.packer = stride, precision, bias is not None, act, slope, packer
        return out.permute(0, 3, 1, 2)                    # (B,Cout,Ho,Wo), channels_last in memory

    @staticmethod
    def backward(ctx, gy):
        xv, w, y, bias = ctx.saved_tensors
        stride, precision = ctx.stride, ctx.precision
        cout, cin, k, _ = w.shape
        B, H, W, _ = xv.shape
        gyv = _nhwc(gy.float())
        L = hip.lib()
        st = hip.stream_ptr()
        if ctx.act != hip.ACT_NONE:                       # gradient at the pre-activation, from the saved output
            gp = torch.empty_like(gyv)
            hip.check(L.fcvsr_act_bwd(gyv.data_ptr(), y.data_ptr(), gp.data_ptr(), ctx.slope if ctx.act == hip.ACT_LEAKY else 0.0,
                                      gyv.numel(), st), "fcvsr_act_bwd")
            gyv = gp
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # dL/dx = "same" stride-1 convolution of dL/dy (zero-inserted for stride 2) with the transposed, tap-flipped weight
            g_in = gyv
            if stride != 1:
                g_in = torch.zeros((B, H, W, cout), dtype=torch.float32, device=gyv.device)
                g_in[:, ::stride, ::stride, :][:, :gyv.shape[1], :gyv.shape[2]] = gyv
            gx = _run_conv(g_in, w, None, 1, precision, ctx.packer, transposed=True).permute(0, 3, 1, 2)
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            (dw,), acc_w, (gw,) = grad_destinations(w)
            if cout == 1 and k == 3 and stride == 1 and cin in (16, 32, 64):
                # one output channel (conv_last0): x is read once, 9 x cin accumulators per thread
                n = L.fcvsr_wgrad_cout1_scratch_elems(B, H, cin)
                scratch = torch.empty(n, dtype=torch.float32, device=xv.device)
                hip.check(L.fcvsr_wgrad_cout1(xv.data_ptr(), gyv.data_ptr(), B, H, W, cin, dw.data_ptr(), scratch.data_ptr(), n, acc_w, st),
                          "fcvsr_wgrad_cout1")
            elif precision in _MMA and L.fcvsr_conv2d_wgrad_mfma_eligible(cin, cout, k, k, stride, k // 2):
                # 16-bit modes, 3x3 / 1x1 layers with multiples of 64 channels: products on the matrix cores; the kernel has every gy tile
                # in registers, so it also sums gy's columns (the bias gradient)
                n = L.fcvsr_conv2d_wgrad_mfma_scratch_elems(B, H, W, cin, cout, k, k)
                scratch = torch.empty(n, dtype=torch.float32, device=xv.device)
                (db,), acc_b, (gb,) = grad_destinations(bias) if need_b else ((None,), 0, (None,))
                xd, gd = hip.view(xv), hip.view(gyv)
                hip.check(L.fcvsr_conv2d_wgrad_mfma(C.addressof(xd), C.addressof(gd), B, H, W, k, k, stride, k // 2, dw.data_ptr(), hip.ptr(db),
                                                    scratch.data_ptr(), n, acc_w, acc_b, st), "fcvsr_conv2d_wgrad_mfma")
                need_b = False
            else:
                Ho, Wo = gyv.shape[1], gyv.shape[2]
                n = L.fcvsr_conv2d_wgrad_scratch_elems(B, Ho, Wo, cin, cout, k, k)
                scratch = torch.empty(n, dtype=torch.float32, device=xv.device)
                xd, gd = hip.view(xv), hip.view(gyv)
                hip.check(L.fcvsr_conv2d_wgrad(C.addressof(xd), C.addressof(gd), B, H, W, k, k, stride, k // 2, dw.data_ptr(), scratch.data_ptr(),
                                               n, acc_w, st), "fcvsr_conv2d_wgrad")
        if need_b:
            (db,), acc_b, (gb,) = grad_destinations(bias)
            _colsum(gyv, db, acc_b)
        return gx, gw, gb, None, None, None, None, None


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, precision: str = "f32",
           act: Optional[str] = None, slope: float = 0.0, packer: Optional[WeightPacker] = None) -> torch.Tensor:
    """act(nn.Conv2d(k, stride, padding=k//2)(x)) with HIP forward / input-gradient / weight-gradient kernels; `act` in
    {None, "relu", "lrelu"} (slope) is evaluated in the forward kernel's epilogue and differentiated from the saved output.
    `packer`: the WeightPacker of the training pass in progress (None: the 16-bit weight operands are packed per call).
    CUDA (HIP) tensors only: there is no CPU fallback."""
    if not x.is_cuda:
        raise RuntimeError("fcvsr_amd.train.conv2d needs device tensors (the HIP path has no CPU fallback)")
    return _Conv2dFn.apply(x, w, bias, stride, precision, _ACT[act], float(slope), packer)


class _ConvLevelsFn(torch.autograd.Function):
    """One nn.Conv2d applied to several tensors of different sizes (the pyramid levels of a BlockRCB layer, reference
    CVSR_freq.py:766-777) as ONE forward launch, ONE input-gradient launch, and one matrix-core weight-gradient launch per level with a
    single ordered reduction that also yields the bias gradient - instead of three independent layers whose gradients autograd adds.
    16-bit modes, stride 1, cin and cout multiples of 64 (the wrapper checks)."""

    @staticmethod
    def forward(ctx, w, bias, precision, act, slope, packer, *xs):
        mdt, tdt = _MMA[precision]
        cout, cin, k, _ = w.shape
        xvs = [_nhwc(x.float()) for x in xs]
        outs = [torch.empty((xv.shape[0], xv.shape[1], xv.shape[2], cout), dtype=torch.float32, device=xv.device) for xv in xvs]
        b = None if bias is None else bias.detach().float().contiguous()
        hip.conv2d_mfma([dict(srcs=[xv], dst=o) for xv, o in zip(xvs, outs)], _packed(packer, w, tdt, False), k, cout, mdt, bias=b,
                        act=act, slope=slope)
        ctx.save_for_backward(w, bias, *xvs, *(outs if act != hip.ACT_NONE else []))
        ctx.n, ctx.precision, ctx.has_bias, ctx.act, ctx.slope, ctx.packer = len(xs), precision, bias is not None, act, slope, packer
        return tuple(o.permute(0, 3, 1, 2) for o in outs)

    @staticmethod
    def backward(ctx, *gys):
        n = ctx.n
        w, bias = ctx.saved_tensors[0], ctx.saved_tensors[1]
        xvs = ctx.saved_tensors[2:2 + n]
        ys = ctx.saved_tensors[2 + n:]
        mdt, tdt = _MMA[ctx.precision]
        cout, cin, k, _ = w.shape
        L = hip.lib()
        st = hip.stream_ptr()
        gvs = []
        for i, gy in enumerate(gys):
            gv = _nhwc(gy.float())
            if ctx.act != hip.ACT_NONE:
                gp = torch.empty_like(gv)
                hip.check(L.fcvsr_act_bwd(gv.data_ptr(), ys[i].data_ptr(), gp.data_ptr(), ctx.slope if ctx.act == hip.ACT_LEAKY else 0.0,
                                          gv.numel(), st), "fcvsr_act_bwd")
                gv = gp
            gvs.append(gv)
        gxs = [None] * n
        if any(ctx.needs_input_grad[6:]):
            gx = [torch.empty_like(xv) for xv in xvs]
            hip.conv2d_mfma([dict(srcs=[gv], dst=o) for gv, o in zip(gvs, gx)], _packed(ctx.packer, w, tdt, True), k, cin, mdt)
            gxs = [o.permute(0, 3, 1, 2) for o in gx]
        gw = gb = None
        need_w, need_b = ctx.needs_input_grad[0], ctx.has_bias and ctx.needs_input_grad[1]
        if need_w or need_b:                              # (the bias gradient comes out of the weight-gradient kernel)
            Bs = (C.c_int * n)(*[xv.shape[0] for xv in xvs])
            Hs = (C.c_int * n)(*[xv.shape[1] for xv in xvs])
            Ws = (C.c_int * n)(*[xv.shape[2] for xv in xvs])
            ne = L.fcvsr_conv2d_wgrad_mfma_groups_scratch_elems(Bs, Hs, Ws, n, cin, cout, k, k)
            scratch = torch.empty(ne, dtype=torch.float32, device=w.device)
            if need_w:
                (dw,), acc_w, (gw,) = grad_destinations(w)
            else:
                dw, acc_w = torch.empty(w.shape, dtype=torch.float32, device=w.device), 0
            (db,), acc_b, (gb,) = grad_destinations(bias) if need_b else ((None,), 0, (None,))
            xd = (hip.View * n)(*[hip.view(xv) for xv in xvs])
            gd = (hip.View * n)(*[hip.view(gv) for gv in gvs])
            hip.check(L.fcvsr_conv2d_wgrad_mfma_groups(xd, gd, Bs, Hs, Ws, n, k, k, k // 2, dw.data_ptr(), hip.ptr(db), scratch.data_ptr(), ne,
                                                       acc_w, acc_b, st), "fcvsr_conv2d_wgrad_mfma_groups")
        return (gw, gb, None, None, None, None, *gxs)


def conv2d_levels(xs, w: torch.Tensor, bias: Optional[torch.Tensor] = None, precision: str = "f32", act: Optional[str] = None,
                  slope: float = 0.0, packer: Optional[WeightPacker] = None):
    """[act(conv(x)) for x in xs] for ONE stride-1 layer applied to up to three tensors (pyramid levels): grouped launches in the 16-bit
    modes when the layer takes the matrix-core path in every direction; otherwise a plain loop over `conv2d`."""
    xs = list(xs)
    cout, cin, k, _ = w.shape
    ok = (precision in _MMA and 1 < len(xs) <= 3 and k in (1, 3) and cin % 64 == 0 and cout % 64 == 0 and all(x.is_cuda for x in xs))
    if ok:
        ok = hip.mfma_eligible(k, 1, [dict(srcs=[_nhwc(x.float())], dst=_nhwc(x.float())) for x in xs])
    if not ok:
        return [conv2d(x, w, bias, 1, precision, act, slope, packer) for x in xs]
    return list(_ConvLevelsFn.apply(w, bias, precision, _ACT[act], float(slope), packer, *xs))
