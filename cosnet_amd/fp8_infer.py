"""Static-scale fp8 (OCP e4m3) encoders for whole-sequence inference.

The fp8 training path (cosnet_amd/fp8.py) scales activations with DELAYED scaling: every encoder
pass quantises with the previous pass's amax and then advances the scale, so a frame's features
depend on which frames were encoded before it and a feature bank of them is not well defined.
Here the scales are calibrated once and frozen:

* calibrate() runs the bf16 encoders over some frames and records, for every tensor an fp8 conv
  reads, the maximum of |x| over all of them (cn_fp8_quant_fmt mode 2: an integer atomicMax on
  the float bits, so the result is exact and independent of chunking and frame order).
* Fp8Calibration holds those maxima under names built from named_modules() paths and
  round-trips through JSON bit for bit.
* model.set_fp8_static(calib) turns them into one frozen state table per encoder
  (scale = amax * margin / 448 by cn_fp8_update, as the delayed path computes it) and quantises
  every eligible conv weight once with current scaling.
* encode_frames_static() walks one encoder in the layer order of EncoderPairFn.forward (one
  segment, running statistics).  Every eligible conv -- the convs conv_bn would run in fp8, by
  fp8.fp8_conv_ok: a bf16 input of 16-channel multiples and more than FP8_MIN_ROWS rows -- is
  cn_conv_fwd_fp8 on an e4m3 image written by its producer's cn_bn_apply_q8 (the stem / maxpool
  output and the pooled rows of the ASPP concat, which no BN apply produces, by
  cn_fp8_quant_static).  A bottleneck's y1 and y2 and the ASPP's 2560-wide concat exist as e4m3
  only; block outputs as bf16 (the residual) and e4m3.  No launch of the walk writes a scale
  state, so a frame's features depend on the frame, the weights and the calibration alone.

One state per tensor: a block's input, read by its conv1 and its downsample conv, has one
("<block>.x"); so have its y1 and y2, the ASPP's input ("aspp.x") and the whole concat
("aspp.cat").

set_fp8_static(calib, fold_bn=True) also folds every eval-mode BatchNorm into its conv's GEMM:
bottleneck_static_folded / aspp_static_folded run each conv + BN pair as ONE launch,
cn_conv_fwd_fp8_affine (gemm.hip EPI 4 on e4m3 operands), whose epilogue applies the BN's
(scale, shift) table (bn_fold.FoldTables), the residual add and the activation and writes the
bf16 result and / or its e4m3 image under the consumer's frozen state.  No raw conv output is
written and cn_bn_eval_params / cn_bn_apply_q8 do not run.
"""
import json
import weakref

import torch

from . import encoder_fn as E
from . import ops
from .fp8 import FP8_MIN_ROWS, Fp8Weights, fp8_ok, fp8_rows_ok
from .ops import WCACHE

FORMAT = "cosnet_amd.fp8_calibration"
FORMAT_VERSION = 1
ENCODERS = ("encoder", "depth_encoder")


def _paths(enc):
    """id(module) -> its named_modules() path (the id only looks the path up in this process)."""
    return {id(m): name for name, m in enc.named_modules()}


def state_names(enc):
    """The names of one encoder's fp8 activation states, in walk order."""
    paths = _paths(enc)
    names = []
    for blk in E.blocks(enc):
        names += [paths[id(blk)] + s for s in (".x", ".y1", ".y2")]
    return names + [paths[id(enc.aspp)] + ".x", paths[id(enc.aspp)] + ".cat"]


def fp8_conv_weights(enc):
    """The weights of the convs the static walk runs in fp8."""
    ws = []
    for blk in E.blocks(enc):
        ws += [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight]
        if blk.downsample is not None:
            ws.append(blk.downsample[0].weight)
    ws += [cm.weight for cm, _, _, _ in E.aspp_branches(enc.aspp)] + [enc.aspp.bottleneck.weight]
    return ws


# ---- the calibration record ----------------------------------------------------------------------
class Fp8Calibration:
    """amax = {"encoder": {name: max |x|}, "depth_encoder": {...}} (fp32 values held as Python
    floats), the scale margin and a format version.  A file of its own: the {"epoch", "model"}
    snapshot does not change."""

    def __init__(self, amax, margin=1.0, version=FORMAT_VERSION):
        if version != FORMAT_VERSION:
            raise ValueError("fp8 calibration: format version %r, this build reads %d"
                             % (version, FORMAT_VERSION))
        if not isinstance(amax, dict) or set(amax) != set(ENCODERS):
            raise ValueError("fp8 calibration: tables for %s are expected" % (ENCODERS,))
        self.amax = {k: {str(n): float(v) for n, v in amax[k].items()} for k in ENCODERS}
        for tab in self.amax.values():
            for n, v in tab.items():
                if not (v >= 0.0) or v == float("inf"):
                    raise ValueError("fp8 calibration: amax of %s is %r" % (n, v))
        self.margin = float(margin)
        if not self.margin > 0.0:
            raise ValueError("fp8 calibration: margin must be positive")
        self.version = version

    def __eq__(self, other):
        return (isinstance(other, Fp8Calibration) and self.amax == other.amax
                and self.margin == other.margin and self.version == other.version)

    def save(self, path):
        # repr of a Python float round-trips, and every fp32 value is a Python float exactly
        with open(path, "w") as fh:
            json.dump({"format": FORMAT, "version": self.version, "margin": self.margin,
                       "amax": self.amax}, fh, indent=1, sort_keys=True)

    @classmethod
    def load(cls, path):
        with open(path) as fh:
            d = json.load(fh)
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise ValueError("%s is not an fp8 calibration file" % path)
        return cls(d.get("amax"), d.get("margin", 1.0), d.get("version"))

    def check_model(self, model):
        """ValueError unless the key sets are exactly the model's state names."""
        for k in ENCODERS:
            want, have = set(state_names(getattr(model, k))), set(self.amax[k])
            if want != have:
                raise ValueError("fp8 calibration does not match the model's %s: %d names missing, "
                                 "%d unknown (e.g. %s)" % (k, len(want - have), len(have - want),
                                                           sorted(want ^ have)[:2]))


def _new_states(n, device):
    return torch.tensor([[1.0, 1.0, 0.0, ops.FMT_MAX[ops.FP8_E4M3]]] * n, dtype=torch.float32,
                        device=device)


def _calib_walk(enc, imgs, states, slot):
    """One bf16 pass of the per-module path's block functions; amax of every fp8-read tensor."""
    paths = _paths(enc)
    dt = torch.bfloat16

    def amax(x, name):
        ops.fp8_quant(x, states[slot[name]], ops.FP8_AMAX)

    with E.no_fp8():
        x, geo = E.stem_fwd(enc.backbone, (imgs,), 1, dt, None)
        for blk in E.blocks(enc):
            name = paths[id(blk)]
            rec = []
            amax(x, name + ".x")
            x, geo = E.bottleneck_fwd(blk, x, geo, 1, rec)
            r = rec.pop()
            amax(r.y1, name + ".y1")
            amax(r.y2, name + ".y2")
        name = paths[id(enc.aspp)]
        amax(x, name + ".x")
        rec = []
        E.aspp_fwd(enc.aspp, x, geo, 1, rec)
        amax(rec.pop().cat, name + ".cat")


@torch.no_grad()
def calibrate(model, rgbs, depths, encode_chunk=8, margin=1.0):
    """Fp8Calibration of `model` from frames rgbs [T,3,H,W] / depths [T,1,H,W] (fp32 NCHW on the
    GPU): the bf16 encoders run over chunks of encode_chunk frames; the result depends on the set
    of frames only."""
    if model.training:
        raise RuntimeError("fp8 calibration runs in eval mode")
    if model.compute_dtype != torch.bfloat16:
        raise ValueError("fp8 calibration needs the bf16 compute dtype")
    if getattr(model, "fp8", None) is not None:
        raise RuntimeError("fp8 calibration runs the bf16 encoders (set_fp8(False))")
    if rgbs.shape[0] != depths.shape[0] or rgbs.shape[0] < 1 or encode_chunk < 1:
        raise ValueError("calibrate: T >= 1 frames of rgb and depth and encode_chunk >= 1 are expected")
    model._set_dtype()
    rgbs, depths = model._prep(rgbs), model._prep(depths)
    amax = {}
    for key, frames in zip(ENCODERS, (rgbs, depths)):
        enc = getattr(model, key)
        names = state_names(enc)
        slot = {n: i for i, n in enumerate(names)}
        states = _new_states(len(names), frames.device)
        for f0 in range(0, frames.shape[0], encode_chunk):
            _calib_walk(enc, frames[f0:f0 + encode_chunk], states, slot)
        col = states[:, 2].cpu().tolist()
        amax[key] = {n: col[i] for i, n in enumerate(names)}
    return Fp8Calibration(amax, margin)


# ---- the frozen context ------------------------------------------------------------------------
class EncoderStatic:
    """One encoder's frozen state table [n][4] = (scale, 1/scale, 0, 448) and its e4m3 weights;
    with fold_bn, also the (scale, shift) table of every BatchNorm2d of the encoder
    (bn_fold.FoldTables: its staleness rule, cn_bn_fold_table)."""

    def __init__(self, enc, amax, margin, device, fold_bn=False):
        self.names = state_names(enc)
        self.slot = {n: i for i, n in enumerate(self.names)}
        self.paths = _paths(enc)
        rows = [[1.0, 1.0, amax[n], ops.FMT_MAX[ops.FP8_E4M3]] for n in self.names]
        self.states = torch.tensor(rows, dtype=torch.float32, device=device)
        # the delayed path's own arithmetic (fp8_update_k): scale = amax * margin / 448, an
        # all-zero tensor keeps scale 1; the only launch that ever writes this table
        ops.fp8_update(self.states, margin)
        self.weights = Fp8Weights()
        for w in fp8_conv_weights(enc):
            if w.shape[1] % 16:   # fp8_ok's channel rule, known before any frame arrives
                raise ValueError("static fp8: a conv of %d input channels cannot take fp8 operands"
                                 % w.shape[1])
            self.weights.get(w)   # quantised now: nothing is calibrated on first use
        self.fold = None
        if fold_bn:
            from .bn_fold import FoldTables
            self.fold = FoldTables(enc)

    def st(self, name):
        return self.states[self.slot[name]]

    def w8(self, w):
        return self.weights.get(w)


class Fp8Static:
    """A model's static fp8 mode (model.set_fp8_static): one EncoderStatic per encoder.  With
    fold_bn the state also owns the fold tables of both encoders and of the two reduce convs' BNs
    of the a-side head (`head`; None otherwise), and the encoders run the folded walk."""

    def __init__(self, model, calib, fold_bn=False):
        calib.check_model(model)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("set_fp8_static: the model must be on the GPU")
        self.calibration = calib
        self.model = weakref.ref(model)
        self.fold_bn = bool(fold_bn)
        if self.fold_bn and model.training:
            raise RuntimeError("set_fp8_static: the BN fold uses running statistics (eval mode)")
        self.encoders = {k: EncoderStatic(getattr(model, k), calib.amax[k], calib.margin, dev, self.fold_bn)
                         for k in ENCODERS}
        self.head = None
        if self.fold_bn:
            from .bn_fold import FoldTables
            self.head = FoldTables(model, modules=[("bn_A", model.bn_A), ("depth_bn", model.depth_bn)])


def _eval_stats(c, bn):
    return ops.bn_stats(c, bn, False)


def bottleneck_static(blk, x, x8, geo, S, out_state):
    """One bottleneck on frozen scales: x [n*h*w][Cin] bf16 (the residual) and its e4m3 image x8
    -> (y bf16, y8 under out_state, (n, oh, ow)).  y1 and y2 exist as e4m3 only."""
    n, h, w = geo
    s, d = blk.stride, blk.dilation
    planes = blk.conv1.weight.shape[0]
    name = S.paths[id(blk)]
    sx, s1, s2 = S.st(name + ".x"), S.st(name + ".y1"), S.st(name + ".y2")
    w18, ws1 = S.w8(blk.conv1.weight)
    c1, oh, ow = ops.conv_fwd_fp8(x8, n, h, w, w18, planes, 1, s, 0, 1, sx, ws1)
    _, y18 = ops.bn_apply_q8(c1, _eval_stats(c1, blk.bn1), blk.bn1, s1, act=1)
    w28, ws2 = S.w8(blk.conv2.weight)
    c2, _, _ = ops.conv_fwd_fp8(y18, n, oh, ow, w28, planes, 3, 1, d, d, s1, ws2)
    _, y28 = ops.bn_apply_q8(c2, _eval_stats(c2, blk.bn2), blk.bn2, s2, act=1)
    w38, ws3 = S.w8(blk.conv3.weight)
    c3, _, _ = ops.conv_fwd_fp8(y28, n, oh, ow, w38, 4 * planes, 1, 1, 0, 1, s2, ws3)
    y = torch.empty_like(c3)
    if blk.downsample is not None:
        bnd = blk.downsample[1]
        wd8, wsd = S.w8(blk.downsample[0].weight)
        cd, _, _ = ops.conv_fwd_fp8(x8, n, h, w, wd8, 4 * planes, 1, s, 0, 1, sx, wsd)
        _, y8 = ops.bn_apply_q8(c3, _eval_stats(c3, blk.bn3), blk.bn3, out_state, act=1, xr=cd,
                                rstats=_eval_stats(cd, bnd), rbn=bnd, out=y)
    else:
        _, y8 = ops.bn_apply_q8(c3, _eval_stats(c3, blk.bn3), blk.bn3, out_state, act=1, res=x, out=y)
    return y, y8, (n, oh, ow)


def aspp_static(mod, x, x8, geo, S):
    """The ASPP on frozen scales: the four branches' applies write the e4m3 concat directly (no
    bf16 concat); its pooled slice is the pooled rows quantised once and broadcast as bytes."""
    n, h, w = geo
    hw = h * w
    P = n * hw
    dt = x.dtype
    name = S.paths[id(mod)]
    sx, sc = S.st(name + ".x"), S.st(name + ".cat")
    pool = torch.empty((n, 2048), dtype=dt, device=x.device)
    ops.avgpool(x, n, hw, 1.0 / hw, pool)
    wcf, _ = WCACHE.get(mod.conv.weight, dt)
    cp, _, _ = ops.conv_fwd(pool, n, 1, 1, wcf, 512, 1, 1, 0, 1, bias=mod.conv.bias)
    yp = ops.bn_apply(cp, _eval_stats(cp, mod.bn_x), mod.bn_x, act=1)
    cat8 = torch.empty((P, 2560), dtype=torch.uint8, device=x.device)
    ops.bcast_rows_u8(ops.fp8_quant_static(yp, sc), n, hw, cat8[:, :512])
    for bi, (cm, bnm, k, dd) in enumerate(E.aspp_branches(mod)):
        w8, ws = S.w8(cm.weight)
        ci, _, _ = ops.conv_fwd_fp8(x8, n, h, w, w8, 512, k, 1, dd, max(dd, 1), sx, ws, bias=cm.bias)
        ops.bn_apply_q8(ci, _eval_stats(ci, bnm), bnm, sc, act=1,
                        out8=cat8[:, 512 * (bi + 1):512 * (bi + 2)])
    wb8, wsb = S.w8(mod.bottleneck.weight)
    cb, _, _ = ops.conv_fwd_fp8(cat8, n, h, w, wb8, 256, 3, 1, 1, 1, sc, wsb, bias=mod.bottleneck.bias)
    return ops.bn_apply(cb, _eval_stats(cb, mod.bn), mod.bn, act=2, prelu=mod.prelu.weight)


# ---- the same walk with every conv + eval BN pair as one launch (set_fp8_static(fold_bn=True)) ----
def _conv8_folded(S, x8, n, h, w, conv, bn, cout, k, stride, pad, dil, x_state, **kw):
    """One fp8 conv + eval BN pair: cn_conv_fwd_fp8_affine on the conv's frozen e4m3 weight and
    the BN's fold table."""
    w8, ws = S.w8(conv.weight)
    sc, sf = S.fold.get(bn)
    return ops.conv_fwd_fp8_affine(x8, n, h, w, w8, cout, k, stride, pad, dil, x_state, ws, sc, sf, **kw)


def bottleneck_static_folded(blk, x, x8, geo, S, out_state):
    """bottleneck_static with the BNs in the conv GEMMs' epilogues, three launches (four with a
    downsample): conv1 and conv2 write y1 / y2 as e4m3 only; the downsample conv writes
    rd = affine(cd) as bf16 with no activation; conv3 takes rd (or x) as its residual and writes
    y (bf16) and its e4m3 image under out_state.  No raw conv output exists."""
    n, h, w = geo
    s, d = blk.stride, blk.dilation
    planes = blk.conv1.weight.shape[0]
    name = S.paths[id(blk)]
    sx, s1, s2 = S.st(name + ".x"), S.st(name + ".y1"), S.st(name + ".y2")
    _, y18, oh, ow = _conv8_folded(S, x8, n, h, w, blk.conv1, blk.bn1, planes, 1, s, 0, 1, sx, act=1,
                                   out_state=s1, want_y=False)
    _, y28, _, _ = _conv8_folded(S, y18, n, oh, ow, blk.conv2, blk.bn2, planes, 3, 1, d, d, s1, act=1,
                                 out_state=s2, want_y=False)
    res = x
    if blk.downsample is not None:
        res, _, _, _ = _conv8_folded(S, x8, n, h, w, blk.downsample[0], blk.downsample[1], 4 * planes,
                                     1, s, 0, 1, sx, act=0)
    y, y8, _, _ = _conv8_folded(S, y28, n, oh, ow, blk.conv3, blk.bn3, 4 * planes, 1, 1, 0, 1, s2, act=1,
                                res=res, out_state=out_state)
    return y, y8, (n, oh, ow)


def aspp_static_folded(mod, x, x8, geo, S):
    """aspp_static with the BNs folded: the pooled 1x1 conv is bf16 (cn_conv_fwd_affine), the four
    branches write their e4m3 slices of the concat in place, the bottleneck conv writes bf16 with
    the PReLU applied."""
    n, h, w = geo
    hw = h * w
    P = n * hw
    dt = x.dtype
    name = S.paths[id(mod)]
    sx, sc = S.st(name + ".x"), S.st(name + ".cat")
    pool = torch.empty((n, 2048), dtype=dt, device=x.device)
    ops.avgpool(x, n, hw, 1.0 / hw, pool)
    wcf, _ = WCACHE.get(mod.conv.weight, dt)
    psc, psf = S.fold.get(mod.bn_x)
    yp, _, _ = ops.conv_fwd_affine(pool, n, 1, 1, wcf, 512, 1, 1, 0, 1, psc, psf, act=1, bias=mod.conv.bias)
    cat8 = torch.empty((P, 2560), dtype=torch.uint8, device=x.device)
    ops.bcast_rows_u8(ops.fp8_quant_static(yp, sc), n, hw, cat8[:, :512])
    for bi, (cm, bnm, k, dd) in enumerate(E.aspp_branches(mod)):
        _conv8_folded(S, x8, n, h, w, cm, bnm, 512, k, 1, dd, max(dd, 1), sx, act=1, bias=cm.bias,
                      out8=cat8[:, 512 * (bi + 1):512 * (bi + 2)], out_state=sc, want_y=False)
    out, _, _, _ = _conv8_folded(S, cat8, n, h, w, mod.bottleneck, mod.bn, 256, 3, 1, 1, 1, sc, act=2,
                                 prelu=mod.prelu.weight, bias=mod.bottleneck.bias)
    return out


def encode_frames_static(enc, imgs):
    """imgs [n,C,H,W] fp32 NCHW on the GPU -> (feats [n*h*w][256] bf16, (n, h, w)): one encoder
    on frozen fp8 scales (model.set_fp8_static).  Eval mode under no_grad.  A static state that
    carries fold tables (set_fp8_static(fold_bn=True)) takes the folded block functions: the same
    walk order, one launch per conv + BN pair."""
    S = getattr(enc, "_cn_fp8_static", None)
    if S is None:
        raise RuntimeError("encode_frames_static: no static fp8 scales (model.set_fp8_static)")
    if enc.training or torch.is_grad_enabled():
        raise RuntimeError("static fp8 is an inference path: eval mode under torch.no_grad()")
    dt = torch.bfloat16
    folded = S.fold is not None
    bottleneck, aspp = ((bottleneck_static_folded, aspp_static_folded) if folded
                        else (bottleneck_static, aspp_static))
    if folded:   # the stem is bf16 either way: conv + BN as the bf16 fold runs it
        from .bn_fold import stem_folded
        x, geo = stem_folded(enc.backbone, imgs, dt, S.fold)
    else:
        with E.no_fp8():   # the stem is not an fp8 conv: as the bf16 path runs it
            x, geo = E.stem_fwd(enc.backbone, (imgs,), 1, dt, None)
    n, h, w = geo
    fh, fw = ops.out_hw(h, w, 1, 2, 0, 1)   # layer2's stride; layers 3-4 keep the size
    if not fp8_rows_ok(n * fh * fw):
        raise ValueError("static fp8: %d feature-map rows; the fp8 convs need more than %d"
                         % (n * fh * fw, FP8_MIN_ROWS))
    blocks = E.blocks(enc)
    if not fp8_ok(x, x.shape[1]):
        raise RuntimeError("static fp8: the stem output cannot take the fp8 layout")
    x8 = ops.fp8_quant_static(x, S.st(S.paths[id(blocks[0])] + ".x"))
    for i, blk in enumerate(blocks):
        nxt = S.paths[id(blocks[i + 1] if i + 1 < len(blocks) else enc.aspp)] + ".x"
        x, x8, geo = bottleneck(blk, x, x8, geo, S, S.st(nxt))
    return aspp(enc.aspp, x, x8, geo, S), geo
