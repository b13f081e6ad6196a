"""Eval-mode BatchNorm folded into the conv GEMMs for whole-sequence inference.

In eval mode every BatchNorm2d is a frozen per-channel affine.  The default feature-bank walk
(encoder.features_nhwc) still runs each conv + BN pair as three launches: the conv GEMM writes the
raw output c, cn_bn_eval_params rebuilds mean / invstd from the running statistics, and the apply
reads c (and the residual) and writes y.  Here

* FoldTables(enc) holds one (scale, shift) pair per BatchNorm2d of an encoder, written once by
  cn_bn_fold_table (the apply's own fp32 arithmetic) and rebuilt when one of the BN's four tensors
  changed (torch's version counters);
* encode_frames_folded() walks one encoder in the layer order of EncoderPairFn.forward (one
  segment, running statistics) with every conv + BN pair as ONE launch, cn_conv_fwd_affine: the
  GEMM epilogue (gemm.hip EPI 4; gemm_ws.hip FOLD for the shallow-K wide 1x1 convs) applies the
  affine, the bottleneck's residual add and the activation before the one rounding.  No raw conv output exists in memory.  A downsample block's downsample conv
  writes rd = affine(cd) with no activation and conv3 takes it as its residual; the ASPP's
  branches write their slices of the concat in place; the ASPP bottleneck conv (split over K)
  applies the affine and the PReLU in its reduce.

In fp32 the walk is bitwise encoder.features_nhwc (tests/test_gpu_bn_fold.py): the same GEMM
accumulators, the same affine, one rounding either way.  In bf16 it rounds once where the
default path rounds twice (c, then y), and a downsample block's rd is rounded to bf16 where the
default apply adds it in fp32.

model.set_bn_fold() switches FeatureBank.encode / segment_sequence to this walk and
head_a_indexed to folded reduce convs.
"""
import weakref

import torch
import torch.nn as nn

from . import _native as nv
from . import encoder_fn as E
from . import ops
from .ops import WCACHE

ENCODERS = ("encoder", "depth_encoder")

FOLDED, UNFOLDED = "folded", "unfolded"


# (M, Cout, K, dilation) of the classes tools/bn_fold_probe.py did NOT measure faster folded than
# as today's three launches by more than the spread of its repeated runs
# (profiles/r12_bn_fold_classes.txt: both encoders at 473 x 473, encode_chunk 8, bf16).  One class:
# the depth ASPP's dilation-7 branch, 3.7 % faster folded against a 5.1 % spread.  Its five siblings
# of the same GEMM shape measured 2.5-3.6 % faster against spreads of 0.5-2.5 %.
_NOT_FASTER = {(28800, 512, 18432, 7)}


def fold_route(m, cout, kdim, dil=1, res=False):
    """How one conv + eval BN class runs in the folded walk: FOLDED -- cn_conv_fwd_affine, which
    the dispatcher puts on the weight-stationary kernel's folded epilogue for the shapes that
    kernel serves (K <= 256 into 4 K channels, M >= 8192: conv3 of layers 1-3 and layer 1's
    downsample conv, measured 2.0-3.1x faster there than on the generic epilogue), on the generic
    GEMM epilogue otherwise, or on the split-K reduce -- or UNFOLDED (conv_fwd + bn_stats +
    bn_apply, as the default walk).  A class is folded only where tools/bn_fold_probe.py measured
    it faster than today's three launches by more than the spread of the repeated runs; a shape
    that was not measured (another frame size or chunk) is folded."""
    return UNFOLDED if (m, cout, kdim, dil) in _NOT_FASTER else FOLDED


def _bn_tensors(bn):
    return [t for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias) if t is not None]


class FoldTables:
    """(scale, shift) of every BatchNorm2d under `root`, keyed by its named_modules() path and
    written by cn_bn_fold_table.  get() checks the version counters and storage of the BN's four
    tensors and rewrites a stale pair IN PLACE, so load_state_dict or an optimiser step after
    the tables were built is followed."""

    def __init__(self, root, modules=None):
        self.paths = {}
        self._tab = {}    # path -> fp32 [2, C]: scale, shift
        self._tag = {}
        for name, m in (modules if modules is not None else root.named_modules()):
            if isinstance(m, nn.BatchNorm2d):
                if m.running_mean is None:
                    raise ValueError("bn fold: %s keeps no running statistics" % name)
                self.paths[id(m)] = name
                self._build(name, m)

    @staticmethod
    def tag_of(bn):
        return tuple((t._version, t.data_ptr()) for t in _bn_tensors(bn)) + (float(bn.eps),)

    def _build(self, name, bn):
        tab = self._tab.get(name)
        if tab is None or tab.device != bn.running_mean.device:
            tab = torch.empty((2, bn.running_mean.shape[0]), dtype=torch.float32, device=bn.running_mean.device)
            self._tab[name] = tab
        ops.bn_fold_table(bn, out=tab)
        self._tag[name] = self.tag_of(bn)

    def stale(self, bn):
        return self._tag[self.paths[id(bn)]] != self.tag_of(bn)

    def get(self, bn):
        """(scale, shift) fp32 [C] of `bn`, current with its tensors."""
        name = self.paths[id(bn)]
        if self.stale(bn):
            self._build(name, bn)
        t = self._tab[name]
        return t[0], t[1]

    def __len__(self):
        return len(self.paths)


def _tables(enc):
    T = getattr(enc, "_cn_bn_fold", None)
    if T is None:
        raise RuntimeError("encode_frames_folded: no fold tables (model.set_bn_fold())")
    return T


def conv_bn_folded(T, x, n, h, w, wf, cout, k, stride, pad, dil, bn, act=0, prelu=None, res=None,
                   bias=None, out=None):
    """One conv + eval BN (+ residual, + activation) -> (y, oh, ow), by fold_route."""
    oh, ow = ops.out_hw(h, w, k, stride, pad, dil)
    if fold_route(n * oh * ow, cout, wf.shape[1], dil, res is not None) == FOLDED:
        sc, sf = T.get(bn)
        return ops.conv_fwd_affine(x, n, h, w, wf, cout, k, stride, pad, dil, sc, sf, act=act, prelu=prelu,
                                   res=res, bias=bias, out=out)
    c, oh, ow = ops.conv_fwd(x, n, h, w, wf, cout, k, stride, pad, dil, bias=bias)
    y = ops.bn_apply(c, ops.bn_stats(c, bn, False), bn, act=act, prelu=prelu, res=res, out=out)
    return y, oh, ow


def stem_folded(res, imgs, dt, T):
    n, cimg, h, w = imgs.shape
    x = torch.empty((n * h * w, 8), dtype=dt, device=imgs.device)
    nv.call("cn_nchw_to_nhwc", nv.dtype_code(dt), imgs.data_ptr(), n, cimg, h, w, 8, x.data_ptr(), nv.stream())
    wf, _ = WCACHE.get(res.conv1.weight, dt, cin_pad=8, need_t=False)
    y, oh, ow = conv_bn_folded(T, x, n, h, w, wf, 64, 7, 2, 3, 1, res.bn1, act=1)
    ph, pw = ops.pool_out(oh), ops.pool_out(ow)
    out = torch.empty((n * ph * pw, 64), dtype=dt, device=x.device)
    am = torch.empty((n * ph * pw * 64,), dtype=torch.uint8, device=x.device)
    nv.call("cn_maxpool_fwd", nv.dtype_code(dt), y.data_ptr(), n, oh, ow, 64, ph, pw, 3, 2, 1,
            out.data_ptr(), am.data_ptr(), nv.stream())
    return out, (n, ph, pw)


def bottleneck_folded(blk, x, geo, T):
    """One bottleneck, three (four with a downsample) launches: x [n*h*w][Cin] -> (y, (n, oh, ow))."""
    n, h, w = geo
    dt = x.dtype
    s, d = blk.stride, blk.dilation
    planes = blk.conv1.weight.shape[0]
    w1f, _ = WCACHE.get(blk.conv1.weight, dt)
    w2f, _ = WCACHE.get(blk.conv2.weight, dt)
    w3f, _ = WCACHE.get(blk.conv3.weight, dt)
    y1, oh, ow = conv_bn_folded(T, x, n, h, w, w1f, planes, 1, s, 0, 1, blk.bn1, act=1)
    y2, _, _ = conv_bn_folded(T, y1, n, oh, ow, w2f, planes, 3, 1, d, d, blk.bn2, act=1)
    res = x
    if blk.downsample is not None:
        wdf, _ = WCACHE.get(blk.downsample[0].weight, dt)
        res, _, _ = conv_bn_folded(T, x, n, h, w, wdf, 4 * planes, 1, s, 0, 1, blk.downsample[1], act=0)
    y, _, _ = conv_bn_folded(T, y2, n, oh, ow, w3f, 4 * planes, 1, 1, 0, 1, blk.bn3, act=1, res=res)
    return y, (n, oh, ow)


def aspp_folded(mod, x, geo, T):
    n, h, w = geo
    hw = h * w
    P = n * hw
    dt = x.dtype
    cat = torch.empty((P, 2560), dtype=dt, device=x.device)
    pool = torch.empty((n, 2048), dtype=dt, device=x.device)
    ops.avgpool(x, n, hw, 1.0 / hw, pool)
    wcf, _ = WCACHE.get(mod.conv.weight, dt)
    yp, _, _ = conv_bn_folded(T, pool, n, 1, 1, wcf, 512, 1, 1, 0, 1, mod.bn_x, act=1, bias=mod.conv.bias)
    nv.call("cn_bcast_rows", ops.dtc(yp), yp.data_ptr(), n, hw, 512, 1.0, cat.data_ptr(), 2560, 0,
            nv.stream())
    for bi, (cm, bnm, k, dd) in enumerate(E.aspp_branches(mod)):
        wf, _ = WCACHE.get(cm.weight, dt)
        conv_bn_folded(T, x, n, h, w, wf, 512, k, 1, dd, max(dd, 1), bnm, act=1, bias=cm.bias,
                       out=cat[:, 512 * (bi + 1):512 * (bi + 2)])
    wbf, _ = WCACHE.get(mod.bottleneck.weight, dt)
    out, _, _ = conv_bn_folded(T, cat, n, h, w, wbf, 256, 3, 1, 1, 1, mod.bn, act=2, prelu=mod.prelu.weight,
                               bias=mod.bottleneck.bias)
    return out


def encode_frames_folded(enc, imgs):
    """imgs [n,C,H,W] fp32 NCHW on the GPU -> (feats [n*h*w][256], (n, h, w)) in the encoder's
    compute dtype: encoder.features_nhwc with every conv + BN pair folded into one launch
    (model.set_bn_fold).  Eval mode under no_grad."""
    T = _tables(enc)
    if enc.training or torch.is_grad_enabled():
        raise RuntimeError("the BN fold is an inference path: eval mode under torch.no_grad()")
    dt = getattr(enc, "_cn_dtype", torch.bfloat16)
    x, geo = stem_folded(enc.backbone, imgs, dt, T)
    for blk in E.blocks(enc):
        x, geo = bottleneck_folded(blk, x, geo, T)
    return aspp_folded(enc.aspp, x, geo, T), geo


class BnFold:
    """A model's BN-fold mode (model.set_bn_fold): one FoldTables per encoder and one for the two
    reduce convs' BNs of the a-side head."""

    def __init__(self, model):
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("set_bn_fold: the model must be on the GPU")
        self.model = weakref.ref(model)
        self.encoders = {k: FoldTables(getattr(model, k)) for k in ENCODERS}
        self.head = FoldTables(model, modules=[("bn_A", model.bn_A), ("depth_bn", model.depth_bn)])
