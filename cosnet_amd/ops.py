"""Tensor-level wrappers over the C ABI (no autograd here).

Activations are 2-D tensors [P, C] = NHWC flattened, possibly a channel-slice view of a
wider buffer (row stride = t.stride(0)).  Every function launches HIP kernels from
libcosnet_hip on the current torch stream; nothing here computes with torch ops.
"""
import collections
import ctypes
import os
import weakref

import torch

from . import _native as nv

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D [P, C] view"
    return t.stride(0)


def dtc(t):
    return nv.dtype_code(t.dtype)


def out_hw(h, w, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1


def pool_out(h, k=3, s=2, p=1):
    """MaxPool2d output size with ceil_mode=True (deeplab/residual_net.py:109)."""
    o = -(-(h + 2 * p - (k - 1) - 1) // s) + 1
    if (o - 1) * s >= h + p:
        o -= 1
    return o


def _ptrs(ts):
    """Host array of the data pointers of tensors `ts` (None: a null pointer)."""
    return (ctypes.c_void_p * len(ts))(*[nv.ptr(t) for t in ts])


# ---- argument groups of the C ABI, each built in one place -----------------------------------
def _mat(t, ld_none=None):
    """(pointer, row stride) of a [P, C] matrix operand, for splatting into a call.  An optional
    operand names ld_none, the stride that goes with its null pointer."""
    return (None, ld_none) if t is None else (t.data_ptr(), ld(t))


def _workspace(dev, size, *query_args, per=1, floor=0, dtype=torch.float32):
    """(ws, n): launch scratch of n units -- n given, or asked of the *_workspace_* query that `size`
    names -- as a tensor of n // per elements (per=4: a byte count held as floats), at least
    `floor`; ws is None, a null pointer to the library, when that is nothing."""
    n = size if isinstance(size, int) else int(nv.query(size, *query_args))
    elems = max(n // per, floor)
    return (torch.empty((elems,), dtype=dtype, device=dev) if elems else None), n


# ---- train-mode BatchNorm bookkeeping shared by bn_stats and the conv + BN epilogues ----------
def _check_train_rows(m, nseg, c):
    """Each of the nseg segments of m rows needs more than one row (torch's own error text)."""
    if m % nseg or m // nseg <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size "
                         "torch.Size([%d, %d, 1, 1])" % (m // nseg, c))


def _momentum(bn):
    return float(bn.momentum if bn.momentum is not None else BN_MOMENTUM)


def _count_batches(bn, nseg):
    """The host-side count of BN batches seen: one per segment, as one reference BN call each."""
    bn._cn_nbt = getattr(bn, "_cn_nbt", 0) + nseg


# ---- optional per-launch timing of the implicit-GEMM kernel (bench.py roofline) -----------
class GemmProfile:
    """Records (algorithmic FLOPs, start, end) HIP events around every implicit-GEMM launch
    on the current stream while active."""

    active = None

    def __init__(self):
        self.rec = []

    def __enter__(self):
        GemmProfile.active = self
        return self

    def __exit__(self, *a):
        GemmProfile.active = None
        return False

    def summary(self):
        """(launches, total FLOPs, total kernel seconds) — call after synchronize()."""
        fl = sum(r[0] for r in self.rec)
        t = sum(r[1].elapsed_time(r[2]) for r in self.rec) * 1e-3
        return len(self.rec), fl, t

    def algorithmic_bytes(self):
        """Total unique operand bytes of the recorded launches: each GEMM's inputs read once
        (the conv input tensor itself, not its implicit im2col) plus its output written once."""
        return sum(r[4] for r in self.rec)

    def select(self, op):
        """(launches, FLOPs, seconds, algorithmic bytes) of the launches whose tag op == `op`."""
        sel = [r for r in self.rec if r[3] is not None and r[3][0] == op]
        return (len(sel), sum(r[0] for r in sel),
                sum(r[1].elapsed_time(r[2]) for r in sel) * 1e-3, sum(r[4] for r in sel))

    def by_tag(self):
        """{tag: [launches, FLOPs, seconds]} -- tag = (op, M, N, K) of each launch."""
        out = {}
        for fl, e0, e1, tag, _ in self.rec:
            r = out.setdefault(tag, [0, 0.0, 0.0])
            r[0] += 1
            r[1] += fl
            r[2] += e0.elapsed_time(e1) * 1e-3
        return out


class _Launch:
    """`with _profiled(...):` around a launch: the record's end event, recorded however the block
    is left."""
    __slots__ = ("e1",)

    def __init__(self, e1):
        self.e1 = e1

    def __enter__(self):
        pass

    def __exit__(self, *a):
        if self.e1 is not None:
            self.e1.record()


_UNPROFILED = _Launch(None)


def _profiled(record, *args):
    """Context of one GemmProfile record; record(*args) -> (flops, tag, nbytes) is worked out only
    while a profile is active, so an unprofiled launch pays for none of it."""
    p = GemmProfile.active
    # ROCm has no timing event nodes in graphs: profile an eager step instead
    if p is None or torch.cuda.is_current_stream_capturing():
        return _UNPROFILED
    flops, tag, nbytes = record(*args)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    p.rec.append((flops, e0, e1, tag, nbytes))
    return _Launch(e1)


# ---- weights -------------------------------------------------------------------------------
class WeightCache:
    """Compute-dtype copies of fp32 master conv weights: [Cout][KH][KW][Cp] for the forward
    GEMM and [Cin][KH][KW][Cout] for dgrad.

    One entry per (parameter, dtype, cin padding), with storage that is allocated once and
    never replaced (a recorded HIP graph keeps reading it).  An entry is valid while its tag
    (torch version counter, `epoch`, data pointer) matches; a stale entry is re-prepared IN
    PLACE.  The SGD kernel rewrites the copies of every parameter it updates in the same
    pass (optim.SGD, cn_sgd) and re-validates the entry (`refreshed`), so a training step
    runs no separate preparation kernels.  Bumping `epoch` invalidates everything."""

    epoch = 0

    def __init__(self):
        self._c = {}

    @staticmethod
    def _tag(w):
        return (w._version, WeightCache.epoch, w.data_ptr())

    def get(self, w, dtype, cin_pad=None, need_t=True):
        key = (id(w), tuple(w.shape), dtype, cin_pad)
        hit = self._c.get(key)
        if hit is not None and hit[0] == self._tag(w) and (hit[2] is not None or not need_t):
            return hit[1], hit[2]
        cout = w.shape[0]
        cin = w.shape[1]
        khw = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
        cp = cin_pad or cin
        if w.dim() == 4:
            assert w.is_contiguous(memory_format=torch.channels_last), "conv weight must be channels_last"
        if hit is None:
            wf = torch.empty((cout, khw * cp), dtype=dtype, device=w.device)
            wt = torch.empty((cin, khw * cout), dtype=dtype, device=w.device) if need_t else None
            hit = [None, wf, wt, weakref.ref(w, lambda _r, k=key: self._c.pop(k, None))]
            self._c[key] = hit
        elif need_t and hit[2] is None:
            hit[2] = torch.empty((cin, khw * cout), dtype=dtype, device=w.device)
        nv.call("cn_weight_prep", nv.dtype_code(dtype), w.data_ptr(), cout, khw, cin, cp,
                hit[1].data_ptr(), nv.ptr(hit[2]), nv.stream())
        hit[0] = self._tag(w)
        return hit[1], hit[2]

    def entries(self, w):
        """[(wf, wt_or_None, cout, khw, cin, cp, entry)] of parameter w."""
        out = []
        for key, e in self._c.items():
            if key[0] == id(w) and e[3]() is w:
                cout, cin = w.shape[0], w.shape[1]
                khw = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
                out.append((e[1], e[2], cout, khw, cin, e[1].shape[1] // khw, e))
        return out

    def refreshed(self, entry):
        """The SGD kernel rewrote this entry from the updated master weights."""
        w = entry[3]()
        entry[0] = self._tag(w) if w is not None else None

    @staticmethod
    def invalidate(entry):
        entry[0] = None


WCACHE = WeightCache()


# ---- convolution ----------------------------------------------------------------------------
# One conv problem, whichever of its three GEMMs runs: M output pixels, K = k*k*cin.
_Conv = collections.namedtuple("_Conv", "n h w cin oh ow cout k M K")


def _fwd_conv(x, n, h, w, wf, cout, k, stride, pad, dil, bias, out, out_dtype):
    """What every forward conv wrapper starts from: (geometry, output -- allocated unless given --,
    the operands its entry point starts with after the dtype, if it takes one)."""
    cin = wf.shape[1] // (k * k)
    oh, ow = out_hw(h, w, k, stride, pad, dil)
    M = n * oh * ow
    if out is None:
        out = torch.empty((M, cout), dtype=out_dtype, device=x.device)
    return (_Conv(n, h, w, cin, oh, ow, cout, k, M, k * k * cin), out,
            (x.data_ptr(), ld(x), n, h, w, cin, wf.data_ptr(), cout, k, k, stride, pad, dil, nv.ptr(bias),
             out.data_ptr(), ld(out), oh, ow))


def _fwd_record(tag, g, es_in, es_out):
    """A forward conv: x and the weights read, y written once."""
    return (2.0 * g.M * g.cout * g.K, (tag, g.M, g.cout, g.K),
            es_in * (g.n * g.h * g.w * g.cin + g.cout * g.K) + es_out * g.M * g.cout)


def _dgrad_conv(dy, n, oh, ow, wt, cin, k, spd, out, h, w, out_dtype):
    """The same for the input-gradient wrappers; spd = (stride, pad, dil), or (pad, dil) for the
    stride-1 entry points."""
    cout = wt.shape[1] // (k * k)
    if out is None:
        out = torch.empty((n * h * w, cin), dtype=out_dtype, device=dy.device)
    return (_Conv(n, h, w, cin, oh, ow, cout, k, n * oh * ow, k * k * cin), out,
            (dy.data_ptr(), ld(dy), n, oh, ow, cout, wt.data_ptr(), cin, k, k, *spd, out.data_ptr(), ld(out),
             h, w))


def _dgrad_record(tag, g, es, es_x, over_input=False):
    """dy and the weights read at es bytes, es_x bytes per element of x; over_input: the FLOPs
    counted over the input pixels (the fp8 record), not the output pixels."""
    P = g.n * g.h * g.w
    return (2.0 * (P if over_input else g.M) * g.cout * g.K, (tag, P, g.cin, g.k * g.k * g.cout),
            es * (g.M * g.cout + g.cout * g.K) + es_x * P * g.cin)


def _wgrad_record(tag, G, es, n, h, w, cin, oh, ow, cout, k):
    M, K = n * oh * ow, k * k * cin
    return (G * 2.0 * M * cout * K, (tag, cout, K, M), G * (es * (n * h * w * cin + M * cout) + 4 * cout * K))


def conv_fwd(x, n, h, w, wf, cout, k, stride, pad, dil, bias=None, out=None):
    """x [n*h*w, >=cin] -> y [n*oh*ow, cout] (or written into `out`)."""
    g, out, args = _fwd_conv(x, n, h, w, wf, cout, k, stride, pad, dil, bias, out, x.dtype)
    with _profiled(_fwd_record, "fwd", g, x.element_size(), x.element_size()):
        nws = fwd_split_floats(x, g.M, cout, g.K)
        if nws:   # deep one-round conv (the ASPP bottleneck): 256x256 tiles split over K
            nv.call("cn_conv_fwd_ws", dtc(x), *args, nv.ptr(_workspace(x.device, nws)[0]), nws, nv.stream())
        else:
            nv.call("cn_conv_fwd", dtc(x), *args, nv.stream())
    return out, g.oh, g.ow


def _fwd_affine_record(tag, g, es, has_res):
    """A forward conv with the eval-mode BN folded in: x and the weights read, the residual read if
    there is one, y written once -- no raw conv output."""
    fl, tg, nb = _fwd_record(tag, g, es, es)
    return fl, tg, nb + (es * g.M * g.cout if has_res else 0)


def conv_fwd_affine(x, n, h, w, wf, cout, k, stride, pad, dil, scale, shift, act=0, prelu=None, res=None,
                    bias=None, out=None):
    """y = act(fma(conv(x) + bias, scale, shift) + res) in one launch (cn_conv_fwd_affine): a conv
    and the eval-mode BatchNorm behind it, scale / shift fp32 [cout] from bn_fold_table; act 0
    none, 1 ReLU, 2 PReLU (prelu[0]); res a [M, cout] view of y's dtype.  x [n*h*w, >=cin] ->
    (y [n*oh*ow, cout] or `out`, oh, ow); the raw conv output is never written."""
    g, out, args = _fwd_conv(x, n, h, w, wf, cout, k, stride, pad, dil, bias, out, x.dtype)
    if res is not None and (res.dtype != out.dtype or tuple(res.shape) != (g.M, cout)):
        raise ValueError("conv_fwd_affine: res must be a [%d, %d] view of the output's dtype" % (g.M, cout))
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != cout or t.stride(0) != 1:
            raise ValueError("conv_fwd_affine: scale / shift are fp32 [%d] arrays" % cout)
    with _profiled(_fwd_affine_record, "fwd_affine", g, x.element_size(), res is not None):
        nws = fwd_split_floats(x, g.M, cout, g.K)
        nv.call("cn_conv_fwd_affine", dtc(x), *args, scale.data_ptr(), shift.data_ptr(), *_mat(res, 0),
                int(act), nv.ptr(prelu), nv.ptr(_workspace(x.device, nws)[0]), nws, nv.stream())
    return out, g.oh, g.ow


def conv_fwd_partial(x, n, h, w, wf, cout, k, stride, pad, dil, bias=None, out=None):
    """The unrounded product of a forward conv (cn_conv_fwd_partial): x [n*h*w, >=cin] in bf16 or
    fp32 -> (y fp32 [n*oh*ow, cout] or `out`, oh, ow) holding the fp32 accumulator (+ bias): one
    term of a conv split by input channels, for conv_fwd_affine_add to add."""
    g, out, args = _fwd_conv(x, n, h, w, wf, cout, k, stride, pad, dil, bias, out, torch.float32)
    if out.dtype != torch.float32:
        raise ValueError("conv_fwd_partial: the output is fp32")
    with _profiled(_fwd_record, "fwd_partial", g, x.element_size(), 4):
        nv.call("cn_conv_fwd_partial", dtc(x), *args, nv.stream())
    return out, g.oh, g.ow


def _fwd_affine_add_record(tag, g, es, nadd):
    """The folded conv with its fp32 addend rows read once per frame they belong to."""
    fl, tg, nb = _fwd_record(tag, g, es, es)
    return fl, tg, nb + 4 * nadd


def conv_fwd_affine_add(x, n, h, w, wf, cout, k, stride, pad, dil, scale, shift, add, add_rows, add_map=None,
                        act=0, prelu=None, bias=None, out=None):
    """y = act(fma(conv(x) + bias + add[f], scale, shift)) in one launch (cn_conv_fwd_affine_add):
    conv_fwd_affine whose epilogue first adds fp32 rows looked up per block of add_rows output rows
    -- block j of y takes rows f*add_rows .. of `add`, f = add_map[j] (int32 on the GPU; None: j).
    add: fp32 [F*add_rows, >=cout] (conv_fwd_partial's output over a bank of F frames).
    x [n*h*w, >=cin] -> (y [n*oh*ow, cout] or `out`, oh, ow)."""
    g, out, args = _fwd_conv(x, n, h, w, wf, cout, k, stride, pad, dil, bias, out, x.dtype)
    if add is not None and add.dtype != torch.float32:
        raise ValueError("conv_fwd_affine_add: add is fp32")
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != cout or t.stride(0) != 1:
            raise ValueError("conv_fwd_affine_add: scale / shift are fp32 [%d] arrays" % cout)
    add_rows = int(add_rows)
    nblk = g.M // add_rows if add_rows > 0 and g.M % add_rows == 0 else 0   # the library refuses the rest
    if add_map is not None and nblk:
        _idx(add_map, nblk)
    nadd = 0 if add is None else min(add.shape[0], g.M) * cout
    with _profiled(_fwd_affine_add_record, "fwd_affine_add", g, x.element_size(), nadd):
        nv.call("cn_conv_fwd_affine_add", dtc(x), *args, scale.data_ptr(), shift.data_ptr(), *_mat(add, 0),
                nv.ptr(add_map), add_rows, int(act), nv.ptr(prelu), nv.stream())
    return out, g.oh, g.ow


def weight_halves(wf, k, out=None):
    """The two input-channel halves of a forward conv weight wf [Cout][k*k*2C] (= [Cout][k][k][2C]):
    (W[..., :C], W[..., C:]), each contiguous [Cout][k*k*C] in wf's dtype -- conv(W, [a | b]) =
    conv(W[..., :C], a) + conv(W[..., C:], b).  `out`: a [2, Cout, k*k*C] tensor to fill in place."""
    cout, kk = wf.shape[0], k * k
    c2 = wf.shape[1] // kk
    if wf.shape[1] != kk * c2 or c2 % 2:
        raise ValueError("weight_halves: a [Cout][%d*%d*2C] weight is expected" % (k, k))
    c = c2 // 2
    if out is None:
        out = torch.empty((2, cout, kk * c), dtype=wf.dtype, device=wf.device)
    rows = wf.view(cout * kk, c2)
    for i in range(2):
        src, dst = rows[:, i * c:(i + 1) * c], out[i].view(cout * kk, c)
        if wf.is_cuda:
            cast_copy(src, dst)
        else:
            dst.copy_(src)
    return out[0], out[1]


class HalfWeightCache:
    """weight_halves of the compute-dtype forward copy of a conv weight (WCACHE.get), under
    WeightCache's rule: one entry per (parameter, dtype) whose storage is allocated once and never
    replaced, valid while the parameter's tag (version counter, epoch, data pointer) matches and
    rewritten IN PLACE when it does not."""

    def __init__(self):
        self._c = {}

    def get(self, w, dtype):
        key = (id(w), tuple(w.shape), dtype)
        hit = self._c.get(key)
        tag = WeightCache._tag(w)
        if hit is not None and hit[0] == tag:
            return hit[1][0], hit[1][1]
        wf, _ = WCACHE.get(w, dtype, need_t=False)
        if hit is None:
            kk = w.shape[2] * w.shape[3]
            buf = torch.empty((2, w.shape[0], kk * (w.shape[1] // 2)), dtype=dtype, device=w.device)
            hit = [None, buf, weakref.ref(w, lambda _r, k=key: self._c.pop(k, None))]
            self._c[key] = hit
        weight_halves(wf, w.shape[2], out=hit[1])
        hit[0] = tag
        return hit[1][0], hit[1][1]


HCACHE = HalfWeightCache()


def bn_fold_table(bn, out=None):
    """(scale, shift) fp32 [C] of an eval-mode BatchNorm2d (cn_bn_fold_table): the affine bn_apply
    forms from the running statistics on every call, written once.  `out`: a [2, C] fp32 tensor
    to fill in place."""
    c = bn.running_mean.shape[0]
    if out is None:
        out = torch.empty((2, c), dtype=torch.float32, device=bn.running_mean.device)
    g, b = _affine(bn)
    nv.call("cn_bn_fold_table", bn.running_mean.data_ptr(), bn.running_var.data_ptr(), nv.ptr(g), nv.ptr(b),
            c, float(bn.eps), out[0].data_ptr(), out[1].data_ptr(), nv.stream())
    return out[0], out[1]


def fwd_split_floats(x, m, cout, kdim):
    """Workspace of the split-K forward (cn_conv_fwd_workspace_floats; 0: the shape does not split)."""
    return int(nv.query("cn_conv_fwd_workspace_floats", dtc(x), m, cout, kdim))


def conv_fwd_bn(x, n, h, w, wf, cout, k, stride, pad, dil, bn, nseg=1, bias=None):
    """Train mode: y = conv(x) (+ bias) and the BN batch statistics of y from the GEMM epilogue
    (cn_conv_fwd_bn: no pass of its own over y).  Returns (y, oh, ow, (mean, invstd)) with
    [nseg*cout] statistics; bn.running_* updated once per segment like bn_stats."""
    g, out, args = _fwd_conv(x, n, h, w, wf, cout, k, stride, pad, dil, bias, None, x.dtype)
    _check_train_rows(g.M, nseg, cout)
    if fwd_split_floats(x, g.M, cout, g.K):
        # split over K: the statistics come from their own pass over the reduced output
        conv_fwd(x, n, h, w, wf, cout, k, stride, pad, dil, bias=bias, out=out)
        return out, g.oh, g.ow, bn_stats(out, bn, True, nseg)
    nws = int(nv.query("cn_conv_fwd_bn_workspace_floats", dtc(x), g.M, cout, g.K))
    ws = _workspace(x.device, nws)[0]
    mean = torch.empty((nseg * cout,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    with _profiled(_fwd_record, "fwd", g, x.element_size(), x.element_size()):
        nv.call("cn_conv_fwd_bn", dtc(x), *args, nseg, nv.ptr(ws), mean.data_ptr(), invstd.data_ptr(),
                nv.ptr(bn.running_mean), nv.ptr(bn.running_var), _momentum(bn), float(bn.eps), nv.stream())
    _count_batches(bn, nseg)
    return out, g.oh, g.ow, (mean, invstd)


def conv_dgrad_bn(dy, n, oh, ow, wt, cin, k, pad, dil, x, stats, bn, dgamma=None, dbeta=None):
    """Stride-1 conv input-gradient fused with the backward reduction of the BN + ReLU whose
    pre-activation x [n*oh*ow, cin] fed the conv (cn_conv_dgrad_bn).  Returns
    (dy_bn [P, cin], dgamma, dbeta): the gradient at the BN output and the BN's parameter
    gradients (= the sums cn_bn_bwd_apply needs)."""
    gm, out, args = _dgrad_conv(dy, n, oh, ow, wt, cin, k, (pad, dil), None, oh, ow, dy.dtype)
    if dgamma is None:
        dgamma = torch.empty((cin,), dtype=torch.float32, device=dy.device)
    if dbeta is None:
        dbeta = torch.empty((cin,), dtype=torch.float32, device=dy.device)
    ws, _ = _workspace(dy.device, "cn_conv_dgrad_bn_workspace_floats", dtc(dy), gm.M, cin, k * k * gm.cout)
    es = dy.element_size()
    g, b = _affine(bn)
    with _profiled(_dgrad_record, "dgrad1", gm, es, 2 * es):
        # the C names of the two sums are sum_dz (= dbeta) and sum_dzxh (= dgamma), in this order
        nv.call("cn_conv_dgrad_bn", dtc(dy), *args, *_mat(x), stats[0].data_ptr(), stats[1].data_ptr(),
                nv.ptr(g), nv.ptr(b), dbeta.data_ptr(), dgamma.data_ptr(), nv.ptr(ws), nv.stream())
    return out, dgamma, dbeta


def bn_bwd_apply(x, dy, stats, bn, dgamma, dbeta, out=None):
    """dx of a train-mode BN + ReLU (mask from x) given its parameter-gradient sums."""
    p, c = x.shape
    if out is None:
        out = torch.empty((p, c), dtype=x.dtype, device=x.device)
    g, b = _affine(bn)
    nv.call("cn_bn_bwd_apply", dtc(x), *_mat(x), *_mat(dy), p, c, stats[0].data_ptr(),
            stats[1].data_ptr(), nv.ptr(g), nv.ptr(b), dbeta.data_ptr(), dgamma.data_ptr(), *_mat(out),
            nv.stream())
    return out


# ---- fp8 (e4m3) operands (BASELINE configs[4]) ------------------------------------------------
FP8_E4M3, FP8_E5M2 = 0, 1
FMT_MAX = {FP8_E4M3: 448.0, FP8_E5M2: 57344.0}


def fp8_state(device, fmt=FP8_E4M3):
    """Per-tensor fp8 scaling state [scale, 1/scale, amax, format max] (cn_fp8_quant_fmt)."""
    return torch.tensor([1.0, 1.0, 0.0, FMT_MAX[fmt]], dtype=torch.float32, device=device)


FP8_DELAYED, FP8_CURRENT, FP8_AMAX = 0, 1, 2


def fp8_quant(x, state, mode=FP8_CURRENT, out=None, fmt=FP8_E4M3):
    """x [P, C] (fp32 / bf16) -> fp8 bytes [P, C] (uint8; e4m3, or e5m2 with fmt=FP8_E5M2)
    scaled by state (see fp8_state)."""
    p, c = x.shape
    if out is None and mode != FP8_AMAX:
        out = torch.empty((p, c), dtype=torch.uint8, device=x.device)
    nv.call("cn_fp8_quant_fmt", dtc(x), fmt, *_mat(x), p, c, *_mat(out, c), state.data_ptr(), mode,
            nv.stream())
    return out


def fp8_update(states, margin=1.0):
    """Turn each state's collected amax into its next scale (states: [n, 4] or [4])."""
    nv.call("cn_fp8_update", states.data_ptr(), states.numel() // 4, float(margin), nv.stream())


def fp8_quant_static(x, state, out=None, fmt=FP8_E4M3):
    """fp8 bytes of x [P, C] under a frozen state (cn_fp8_quant_static): the state is only read."""
    p, c = x.shape
    if out is None:
        out = torch.empty((p, c), dtype=torch.uint8, device=x.device)
    nv.call("cn_fp8_quant_static", dtc(x), fmt, *_mat(x), p, c, *_mat(out), state.data_ptr(), nv.stream())
    return out


def bcast_rows_u8(src, n, hw, out):
    """out[(i*hw + p), :] = src[i, :] over bytes (src [n, C] contiguous, out a [n*hw, C] view)."""
    nv.call("cn_bcast_rows_u8", src.data_ptr(), n, hw, src.shape[1], *_mat(out), nv.stream())
    return out


def conv_dgrad_fp8(dy8, n, oh, ow, wt8, cin, k, pad, dil, h, w, dy_state, w_state, out=None,
                   accumulate=False):
    """dx (bf16) (+)= conv_dgrad(dy8 e5m2, wt8 e4m3) * s_dy * s_w, stride 1 (fp8 mode)."""
    g, out, args = _dgrad_conv(dy8, n, oh, ow, wt8, cin, k, (pad, dil), out, h, w, torch.bfloat16)
    with _profiled(_dgrad_record, "dgrad8", g, 1, 2, True):   # one-byte operands, a two-byte output
        nv.call("cn_conv_dgrad_fp8", *args, int(accumulate), dy_state.data_ptr(), w_state.data_ptr(), nv.stream())
    return out


def conv_fwd_fp8(x8, n, h, w, wf8, cout, k, stride, pad, dil, x_state, w_state, bias=None,
                 out=None):
    """y (bf16) = conv(x8, w8) * sx * sw (+ bias): the fp8 implicit-GEMM conv."""
    g, out, args = _fwd_conv(x8, n, h, w, wf8, cout, k, stride, pad, dil, bias, out, torch.bfloat16)
    with _profiled(_fwd_record, "fwd8", g, 1, 2):
        nv.call("cn_conv_fwd_fp8", *args, x_state.data_ptr(), w_state.data_ptr(), nv.stream())
    return out, g.oh, g.ow


def _fwd8_affine_record(tag, g, has_res, has_y, has_y8):
    """The fp8 conv with the eval-mode BN folded in: one-byte operands, a bf16 residual, and
    whichever of the bf16 output and its e4m3 image the launch writes."""
    fl, tg, nb = _fwd_record(tag, g, 1, 0)
    return fl, tg, nb + g.M * g.cout * (2 * has_res + 2 * has_y + has_y8)


def conv_fwd_fp8_affine(x8, n, h, w, wf8, cout, k, stride, pad, dil, x_state, w_state, scale, shift,
                        act=0, prelu=None, res=None, bias=None, out=None, out8=None, out_state=None,
                        want_y=True):
    """act(fma(conv(x8, w8) * sx * sw + bias, scale, shift) + res) in one launch
    (cn_conv_fwd_fp8_affine): the static-scale fp8 conv and the eval-mode BatchNorm behind it.
    y (bf16 [M, cout]; `out`, or allocated unless want_y is False) is one rounding of the fp32
    value; y8 (e4m3 bytes; `out8`, or allocated) is written when out_state, the FROZEN state of the
    output tensor, is given, and is the image of the fp32 value, not of y.  scale / shift fp32
    [cout] from bn_fold_table; res a bf16 [M, cout] view.  -> (y or None, y8 or None, oh, ow)."""
    cin = wf8.shape[1] // (k * k)
    oh, ow = out_hw(h, w, k, stride, pad, dil)
    g = _Conv(n, h, w, cin, oh, ow, cout, k, n * oh * ow, k * k * cin)
    if out is None and want_y:
        out = torch.empty((g.M, cout), dtype=torch.bfloat16, device=x8.device)
    if out8 is None and out_state is not None:
        out8 = torch.empty((g.M, cout), dtype=torch.uint8, device=x8.device)
    if out is None and out8 is None:
        raise ValueError("conv_fwd_fp8_affine: nothing to write (want_y=False without out_state)")
    if out8 is not None and out_state is None:
        raise ValueError("conv_fwd_fp8_affine: the e4m3 image needs the output's frozen state")
    if res is not None and (res.dtype != torch.bfloat16 or tuple(res.shape) != (g.M, cout)):
        raise ValueError("conv_fwd_fp8_affine: res must be a bf16 [%d, %d] view" % (g.M, cout))
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != cout or t.stride(0) != 1:
            raise ValueError("conv_fwd_fp8_affine: scale / shift are fp32 [%d] arrays" % cout)
    with _profiled(_fwd8_affine_record, "fwd8_affine", g, res is not None, out is not None, out8 is not None):
        nv.call("cn_conv_fwd_fp8_affine", x8.data_ptr(), ld(x8), n, h, w, cin, wf8.data_ptr(), cout, k, k,
                stride, pad, dil, nv.ptr(bias), x_state.data_ptr(), w_state.data_ptr(), scale.data_ptr(),
                shift.data_ptr(), *_mat(res, 0), int(act), nv.ptr(prelu), *_mat(out, 0), *_mat(out8, 0),
                nv.ptr(out_state), oh, ow, nv.stream())
    return out, out8, oh, ow


def conv_dgrad(dy, n, oh, ow, wt, cin, k, stride, pad, dil, h, w, out=None, accumulate=False):
    g, out, args = _dgrad_conv(dy, n, oh, ow, wt, cin, k, (stride, pad, dil), out, h, w, dy.dtype)
    es = dy.element_size()
    with _profiled(_dgrad_record, "dgrad%d" % stride, g, es, es):
        nv.call("cn_conv_dgrad", dtc(dy), *args, int(accumulate), nv.stream())
    return out


def conv_wgrad(x, n, h, w, cin, dy, oh, ow, cout, k, stride, pad, dil, dw=None):
    """fp32 [cout, k*k*cin] weight gradient (channels_last order), fully overwritten."""
    if dw is None:
        dw = torch.empty((cout, k * k * cin), dtype=torch.float32, device=x.device)
    ws, _ = _workspace(x.device, "cn_conv_wgrad_workspace_floats", dtc(x), n, oh, ow, cout, k, k, cin)
    with _profiled(_wgrad_record, "wgrad", 1, x.element_size(), n, h, w, cin, oh, ow, cout, k):
        nv.call("cn_conv_wgrad", dtc(x), *_mat(x), n, h, w, cin, *_mat(dy), oh, ow, cout, k, k, stride, pad,
                dil, dw.data_ptr(), nv.ptr(ws), nv.stream())
    return dw


GROUP_MAX = 24       # cn_conv_wgrad_grouped's problem limit (gemm.h GEMM_MAXG)


def _group_of(jobs, ix, idy):
    """Checks a group of weight-gradient jobs (tuples with x at index ix, dy at idy); returns
    (size, first x, first dy)."""
    if not 1 <= len(jobs) <= GROUP_MAX:
        raise ValueError("1..%d problems per grouped launch" % GROUP_MAX)
    if any(t is None for j in jobs for t in j):
        raise ValueError("grouped weight gradients take no missing tensor")
    x0, dy0 = jobs[0][ix], jobs[0][idy]
    if any(ld(j[ix]) != ld(x0) or ld(j[idy]) != ld(dy0) for j in jobs):
        raise ValueError("grouped weight gradients need equal row strides")
    return len(jobs), x0, dy0


def conv_wgrad_grouped(jobs, n, h, w, cin, oh, ow, cout, k, stride, pad, dil, split=False):
    """Weight gradients of G convs of ONE shape in one launch (cn_conv_wgrad_grouped): jobs =
    [(x, dy, dw)] with x [n*h*w, cin], dy [n*oh*ow, cout] sharing the row strides, dw fp32
    [cout, k*k*cin] (written).  No split-K workspace and no reduce launch.  split=True: the G
    problems also split over K (cn_conv_wgrad_grouped_ws: one GEMM launch + one reduce launch
    for the group), for shapes too small to fill the chip grouped whole."""
    G, x0, dy0 = _group_of(jobs, 0, 1)
    xs, dys, dws = (_ptrs(ts) for ts in zip(*jobs))
    args = (dtc(x0), G, xs, ld(x0), n, h, w, cin, dys, ld(dy0), oh, ow, cout, k, k, stride, pad, dil, dws)
    with _profiled(_wgrad_record, "wgrad", G, x0.element_size(), n, h, w, cin, oh, ow, cout, k):
        ws, nws = _workspace(x0.device, "cn_conv_wgrad_grouped_workspace_floats", dtc(x0), G, n, oh, ow, cout,
                             k, k, cin) if split else (None, 0)
        if nws:
            nv.call("cn_conv_wgrad_grouped_ws", *args, nv.ptr(ws), nws, nv.stream())
        else:
            nv.call("cn_conv_wgrad_grouped", *args, nv.stream())
    return [dw for _, _, dw in jobs]


def conv_wgrad_fp8(jobs, n, h, w, cin, oh, ow, cout, k, stride, pad, dil):
    """fp8 weight gradients of G <= GROUP_MAX convs of ONE shape in one launch (cn_conv_wgrad_fp8,
    BASELINE configs[4]): jobs = [(x8, x_state, dy8, dy_state, dw)] with x8 e4m3 [n*h*w, cin] (the
    fp8 forward conv's input copy), dy8 e5m2 [n*oh*ow, cout] (the fp8 dgrad's output-gradient
    copy), their [4]-float scale states (element 0 = dequantisation scale) and dw fp32
    [cout, k*k*cin] (written).  Split over K into slabs + one reduce launch when small."""
    G, x0, d0 = _group_of(jobs, 0, 2)
    xs, xst, dys, dst, dws = (_ptrs(ts) for ts in zip(*jobs))
    with _profiled(_wgrad_record, "wgrad8", G, 1, n, h, w, cin, oh, ow, cout, k):
        ws, nws = _workspace(x0.device, "cn_conv_wgrad_fp8_workspace_floats", G, n, oh, ow, cout, k, k, cin)
        nv.call("cn_conv_wgrad_fp8", G, xs, ld(x0), n, h, w, cin, dys, ld(d0), oh, ow, cout, k, k, stride,
                pad, dil, dws, xst, dst, nv.ptr(ws), nws, nv.stream())
    return [j[4] for j in jobs]


def as_param_grad(dw_flat, weight):
    """[cout, k*k*cin] fp32 (OHWI order) -> gradient shaped/stided like the channels_last param."""
    if weight.dim() == 2:
        return dw_flat.view(weight.shape)
    co, ci, kh, kw = weight.shape
    return dw_flat.view(co, kh, kw, ci).permute(0, 3, 1, 2)


def colpart_ws(p, c, device):
    """Workspace of the deterministic column reductions (colsum, gate / head backward)."""
    return _workspace(device, "cn_colpart_workspace_floats", p, c, floor=1)[0]


def colsum(x, out=None):
    """fp32 [C] column sums of x [P, C] (bias gradients), fixed-order (bitwise repeatable)."""
    if out is None:
        out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    ws = colpart_ws(x.shape[0], x.shape[1], x.device)
    nv.call("cn_colsum", dtc(x), *_mat(x), x.shape[0], x.shape[1], out.data_ptr(), ws.data_ptr(),
            nv.stream())
    return out


def avgpool(x, n, hw, scale, out):
    """out [n, C] = scale * sum over the hw rows of each image of x [n*hw, C] (C = out width);
    deterministic fixed-order reduction of row-split partials (AdaptiveAvgPool2d(1),
    deeplab/deeplabv3_encoder.py:57; and its backward with scale 1)."""
    c = out.shape[1]
    ws, _ = _workspace(x.device, "cn_avgpool_workspace_floats", dtc(x), n, hw, c, floor=1)
    nv.call("cn_avgpool", dtc(x), *_mat(x), n, hw, c, float(scale), out.data_ptr(), ws.data_ptr(),
            nv.stream())
    return out


GEMM_KC, GEMM_MC = 0, 2


def gemm(a, b, m, n, k, layout_a=GEMM_KC, layout_b=GEMM_KC, lda=None, ldb=None, a_bs=0, b_bs=0,
         out=None, ldc=None, c_bs=0, c_mode=0, batch=1, ka_lim=None, kb_lim=None, out_dtype=None,
         nsplit=1, alpha=1.0, bias=None, tag=None):
    """C[m, n] = alpha * sum_k A[m, k] * B[n, k] (batched via *_bs element strides)."""
    dt = a.dtype
    if out is None:
        out = torch.empty((batch * m, n), dtype=out_dtype or dt, device=a.device)
        ldc = n
        c_bs = m * n
    c_f32 = int(out.dtype == torch.float32)
    ab = (nv.dtype_code(dt), layout_a, layout_b, m, n, k, k if ka_lim is None else ka_lim,
          k if kb_lim is None else kb_lim, a.data_ptr(), lda, a_bs, b.data_ptr(), ldb, b_bs)
    with _profiled(lambda: (2.0 * batch * m * n * (kb_lim if kb_lim is not None else k),
                            (tag or "gemm%d%d" % (layout_a, layout_b), batch * m, n, k),
                            (batch if a_bs else 1) * m * k * a.element_size() +
                            (batch if b_bs else 1) * n * k * b.element_size() +
                            batch * m * n * out.element_size())):
        if nsplit > 1 and c_mode in (0, 1) and batch == 1 and c_f32 and ldc == n:
            # split-K into fp32 slabs + fixed-order reduction (no atomic contention)
            slab = m * n
            ws = torch.empty((nsplit * slab,), dtype=torch.float32, device=a.device)
            nv.call("cn_gemm", *ab, ws.data_ptr(), ldc, 0, 1, 3, float(alpha), None, 1, nsplit, slab,
                    nv.stream())
            nv.call("cn_splitk_reduce", ws.data_ptr(), _nsplit_eff(k, nsplit, dt), slab, slab,
                    out.data_ptr(), int(c_mode == 1), nv.stream())
        else:
            nv.call("cn_gemm", *ab, out.data_ptr(), ldc, c_bs, c_f32, c_mode, float(alpha), nv.ptr(bias),
                    batch, nsplit, 0, nv.stream())
    return out


# ---- fused co-attention (inference) ----------------------------------------------------------
# COSNET_COATT_FUSED=0 keeps the materialised-S path for inference too (A/B, tests)
COATT_FUSED = os.environ.get("COSNET_COATT_FUSED", "1") != "0"


def coatt_fused_ok(dt, c, va, vb):
    """The fused kernel covers bf16, C = 256 and 16-byte aligned rows (every RAA call site)."""
    return (COATT_FUSED and dt == torch.bfloat16 and c == 256 and ld(va) % 8 == 0
            and ld(vb) % 8 == 0 and va.data_ptr() % 16 == 0 and vb.data_ptr() % 16 == 0)


def _coatt_args(vat, va, vb, n, hw, za, zb, idx=()):
    """The operand group every co-attention forward starts with: the three feature matrices, (the
    frame maps of the indexed form,) the pair geometry and the outputs, whose row stride comes
    from za if present, otherwise from zb."""
    return (*_mat(vat), *_mat(va), *_mat(vb), *idx, n, hw, vat.shape[1], nv.ptr(za), nv.ptr(zb),
            ld(za if za is not None else zb))


def _coatt_record(tag, vat, n, hw, nprod, nmat):
    """A co-attention launch over n pairs: nprod x HW^2 C FLOPs per pair and nmat [n*hw, C] matrices
    read or written once."""
    c = vat.shape[1]
    return nprod * n * hw * hw * c, (tag, n, hw, c), nmat * n * hw * c * vat.element_size()


def coatt_fused(vat, va, vb, n, hw, za=None, zb=None):
    """Z_a = softmax_j(S) Vb and Z_b = softmax_i(S)^T Va with S = vat vb^T, never materialised
    (rgbd_segmentation_RAA.py:160-170).  Algorithmic work: 3 x 2 HW^2 C per pair."""
    ndir = (za is not None) + (zb is not None)
    with _profiled(_coatt_record, "coatt_fused", vat, n, hw, 3 * 2.0, 5):   # both directions counted, whatever ndir
        ws, nws = _workspace(vat.device, "cn_coatt_fused_workspace_bytes", n, hw, ndir, per=4)
        nv.call("cn_coatt_fused_fwd_ws", *_coatt_args(vat, va, vb, n, hw, za, zb), nv.ptr(ws), nws,
                nv.stream())
    return za, zb


def _idx(t, p):
    if t is None:
        return None
    if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or t.shape[0] != p or not t.is_contiguous():
        raise ValueError("frame map: a contiguous int32[%d] tensor on the GPU is expected" % p)
    return t.data_ptr()


def coatt_fused_idx(vat, va, vb, ia, ib, p, hw, za=None, zb=None):
    """coatt_fused over feature banks [T*hw, C]: pair i co-attends a-role frame ia[i] (rows of vat /
    va) with b-role frame ib[i] (rows of vb); ia / ib int32[p] on the GPU (None: frame i).  Outputs
    stacked [p*hw, C]; either may be None (rgbd_segmentation_RAA.py:160-170 per pair of
    test.py:287-305, every frame stored once)."""
    ndir = (za is not None) + (zb is not None)
    with _profiled(_coatt_record, "coatt_fused_idx", vat, p, hw, 3 * ndir * 1.0, 3 + ndir):
        ws, nws = _workspace(vat.device, "cn_coatt_fused_workspace_bytes", p, hw, ndir, per=4)
        nv.call("cn_coatt_fused_fwd_idx",
                *_coatt_args(vat, va, vb, p, hw, za, zb, idx=(_idx(ia, p), _idx(ib, p))), nv.ptr(ws), nws,
                nv.stream())
    return za, zb


def gate_cat_idx(z, vbank, iv, p, hw, g, gb=None, out=None):
    """out[i*hw + r] = [z[i*hw + r] * sigmoid(z[i*hw + r] . g + gb) | vbank[iv[i]*hw + r]]
    (rgbd_segmentation_RAA.py:177-186, :228-235), one launch; iv int32[p] on the GPU (None: i)."""
    c = z.shape[1]
    if out is None:
        out = torch.empty((p * hw, 2 * c), dtype=z.dtype, device=z.device)
    nv.call("cn_gate_cat_idx", dtc(z), *_mat(z), *_mat(vbank), _idx(iv, p), p, hw, c,
            g.reshape(-1).data_ptr(), nv.ptr(gb), *_mat(out), nv.stream())
    return out


def gate_fwd(z, g, gb=None, out=None):
    """out = z * sigmoid(z . g + gb) per row (cn_gate_fwd; rgbd_segmentation_RAA.py:177-184,
    :228-235): the gated half of gate_cat_idx's rows on its own, [P, C] in z's dtype."""
    if out is None:
        out = torch.empty((z.shape[0], z.shape[1]), dtype=z.dtype, device=z.device)
    nv.call("cn_gate_fwd", dtc(z), *_mat(z), z.shape[0], z.shape[1], g.reshape(-1).data_ptr(), nv.ptr(gb),
            *_mat(out), None, nv.stream())
    return out


def mean_groups(x, ngroups, n, out=None):
    """x fp32 [ngroups*n, C] contiguous -> [ngroups, C]: cn_mean_rows of every group of n rows
    (test.py:301-305 for all targets of a sequence at once)."""
    c = x.shape[1]
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] != ngroups * n:
        raise ValueError("mean_groups: a contiguous fp32 [ngroups*n, C] tensor is expected")
    if out is None:
        out = torch.empty((ngroups, c), dtype=torch.float32, device=x.device)
    nv.call("cn_mean_groups", x.data_ptr(), ngroups, n, c, out.data_ptr(), nv.stream())
    return out


def hw_pad(hw):
    return (hw + 31) // 32 * 32


def coatt_f8(vat, va, vb, n, hw, za, zb, lse_a=None, lse_b=None):
    """Both co-attention directions with MX-fp8 operands (BASELINE configs[4]: e4m3 bytes + one
    E8M0 exponent per 32 reduction values, the block-scaled 32x32x64 MFMA), softmax statistics
    in fp32; optional per-row log2-sum-exp2 [n, hw_pad(hw)] for the bf16 flash backward."""
    with _profiled(_coatt_record, "coatt_f8_fwd", vat, n, hw, 3 * 2.0, 5):
        ws, nws = _workspace(vat.device, "cn_coatt_f8_workspace_bytes", n, hw, dtype=torch.uint8)
        nv.call("cn_coatt_f8_fwd", *_coatt_args(vat, va, vb, n, hw, za, zb), nv.ptr(lse_a),
                nv.ptr(lse_b), nv.ptr(ws), nws, nv.stream())
    return za, zb


def coatt_f8_bank(vat, va, t, hw):
    """The MX-fp8 images of one modality's feature bank (vat = va W^T and va, [t*hw, 256] bf16):
    per frame the row images of vat (Q role) and va (K) and the V^T tile image of va (V) that
    coatt_f8's prepass writes, built once per sequence (cn_coatt_f8_bank_build) -> uint8 tensor."""
    c = vat.shape[1]
    for x in (vat, va):   # the kernels read t*hw rows of c bf16 values through raw pointers
        if x.dtype != torch.bfloat16 or not x.is_cuda or x.dim() != 2 or x.shape != vat.shape \
                or t < 1 or hw < 1 or x.shape[0] < t * hw or x.stride(1) != 1:
            raise ValueError("coatt_f8_bank: vat / va must be bf16 [>= %d, C] tensors on the GPU" % (t * hw))
    nb = int(nv.query("cn_coatt_f8_bank_bytes", t, hw))
    img = torch.empty((nb,), dtype=torch.uint8, device=vat.device)
    with _profiled(lambda: (0.0, ("coatt_f8_bank_build", t, hw, c), 2 * t * hw * c * vat.element_size() + nb)):
        nv.call("cn_coatt_f8_bank_build", *_mat(vat), *_mat(va), t, hw, c, img.data_ptr(), nb, nv.stream())
    return img


def coatt_f8_idx(img, img2, t, ia, ib, p, hw, za, za2=None):
    """Z_a of p pairs with MX-fp8 operands over image banks of t frames (coatt_f8_bank): pair i
    reads its queries at frame ia[i] and its keys / values at frame ib[i]; ia / ib int32[p] on the
    GPU (None: frame i).  img2 / za2 (both or neither): a second modality with the same maps, run
    in the same launch (cn_coatt_f8_fwd_idx).  Outputs stacked [p*hw, 256] bf16."""
    c = za.shape[1]
    if (img2 is None) != (za2 is None):
        raise ValueError("coatt_f8_idx: img2 and za2 go together")
    nmod = 1 if img2 is None else 2
    if za2 is not None and (ld(za2) != ld(za) or za2.shape[1] != c):
        raise ValueError("coatt_f8_idx: za and za2 must share their shape and row stride")
    nb = int(nv.query("cn_coatt_f8_bank_bytes", t, hw))
    for im in (img, img2)[:nmod]:
        if im.dtype != torch.uint8 or not im.is_cuda or not im.is_contiguous() or im.numel() < nb:
            raise ValueError("coatt_f8_idx: an image bank of coatt_f8_bank(., ., %d, %d) is expected" % (t, hw))
    # a side only: 2 products of 2 P HW^2 C per modality; operands are one byte per value
    with _profiled(lambda: (nmod * 2 * 2.0 * p * hw * hw * c, ("coatt_f8_fwd_idx", p, hw, c),
                            nmod * (3 * p * hw * c + p * hw * c * za.element_size()))):
        nv.call("cn_coatt_f8_fwd_idx", img.data_ptr(), nv.ptr(img2), t, _idx(ia, p), _idx(ib, p), p, hw,
                c, za.data_ptr(), nv.ptr(za2), ld(za), nv.stream())
    return za, za2


def coatt_f8_train(vat, va, vb, n, hw, za, zb, lse_a, lse_b):
    """Training forward of both directions with MX-fp8 operands (configs[4]): Z_a, Z_b, the
    per-row log2-sum-exp2 normalisers, and the decoded operands (vat_q, va_q, vb_q) -- bf16,
    exact -- that the flash backward recomputes S and P from (cn_coatt_f8_train_fwd)."""
    c = vat.shape[1]
    q = [torch.empty((n * hw, c), dtype=torch.bfloat16, device=vat.device) for _ in range(3)]
    with _profiled(_coatt_record, "coatt_f8_train_fwd", vat, n, hw, 3 * 2.0, 5):
        ws, nws = _workspace(vat.device, "cn_coatt_f8_train_workspace_bytes", n, hw, dtype=torch.uint8)
        nv.call("cn_coatt_f8_train_fwd", *_coatt_args(vat, va, vb, n, hw, za, zb), lse_a.data_ptr(),
                lse_b.data_ptr(), q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), c, nv.ptr(ws), nws,
                nv.stream())
    return tuple(q)


def coatt_flash_fwd(vat, va, vb, n, hw, za, zb, lse_a, lse_b):
    """Training forward of both co-attention directions (S never in HBM) + the per-row
    log2-sum-exp2 normalisers [n, hw_pad(hw)] the backward recomputes P from."""
    with _profiled(_coatt_record, "coatt_flash_fwd", vat, n, hw, 3 * 2.0, 5):
        ws, nws = _workspace(vat.device, "cn_coatt_fused_workspace_bytes", n, hw, 2, per=4)
        nv.call("cn_coatt_flash_fwd_ws", *_coatt_args(vat, va, vb, n, hw, za, zb), lse_a.data_ptr(),
                lse_b.data_ptr(), nv.ptr(ws), nws, nv.stream())


def coatt_flash_bwd(vat, va, vb, wf, za, zb, lse_a, lse_b, dza, dzb, n, hw, dva=None,
                    dva_accumulate=False):
    """Backward of the flash co-attention: returns dVa_t [P, C] (bf16) and, if `dva` is given,
    accumulates dV_a's softmax-over-i term sum_j P1[i][j] dZ_b[j] into it.  Algorithmic work
    (the reference's autograd; the recomputed S is not counted): dP0 = dZa Vb^T
    and/or dP1 = Va dZb^T plus dVa_t = dS Vb in the dVa_t kernel, P1^T dZb in the PV kernel --
    4 x 2 HW^2 C per pair with both gradients, 2 with dZa only."""
    c = vat.shape[1]
    P = n * hw
    hwp = hw_pad(hw)
    dev = vat.device
    d0 = d1 = None
    if dza is not None:
        d0 = torch.empty((P,), dtype=torch.float32, device=dev)
        nv.call("cn_rowdot", dtc(dza), *_mat(dza), *_mat(za), P, c, d0.data_ptr(), nv.stream())
    if dzb is not None:
        d1 = torch.empty((n * hwp,), dtype=torch.float32, device=dev)
        nv.call("cn_rowdot_seg", dtc(dzb), *_mat(dzb), *_mat(zb), P, c, hw, hwp, d1.data_ptr(), nv.stream())
    dvat = torch.empty((P, c), dtype=vat.dtype, device=dev)
    nterm = (dza is not None) + (dzb is not None)
    with _profiled(_coatt_record, "coatt_flash_bwd", vat, n, hw, (1 + nterm) * 2.0, 2 + 2 * nterm):
        # one workspace for the key-split partials of both kernels (they run one after the other)
        ws, nws = _workspace(dev, max(int(nv.query("cn_coatt_flash_bwd_workspace_bytes", n, hw)),
                                      int(nv.query("cn_coatt_fused_workspace_bytes", n, hw, 1))
                                      if dva is not None else 0), per=4)
        nv.call("cn_coatt_flash_dvat_ws", *_mat(vat), *_mat(va), *_mat(dza, c), *_mat(vb),
                *_mat(dzb, c), lse_a.data_ptr(), nv.ptr(d0), lse_b.data_ptr(), nv.ptr(d1), n, hw, c,
                *_mat(dvat), 0, nv.ptr(ws), nws, nv.stream())
    if dva is not None and dzb is not None:
        with _profiled(_coatt_record, "coatt_flash_bwd", vat, n, hw, 2.0, 3):
            nv.call("cn_coatt_flash_pv_ws", *_mat(vat), *_mat(vb), *_mat(dzb), lse_b.data_ptr(), n, hw, c,
                    *_mat(dva), int(dva_accumulate), nv.ptr(ws), nws, nv.stream())
    return dvat


def _nsplit_eff(k, nsplit, dt):
    """Number of splits cn_gemm really launches (chunks rounded up to whole K tiles)."""
    bk = 64 if dt == torch.bfloat16 else 32
    chunk = -(-k // nsplit)
    chunk = -(-chunk // bk) * bk
    return -(-k // chunk)


# ---- batch norm -------------------------------------------------------------------------------
def _ws(dtype, p, c, device, nseg=1):
    return _workspace(device, "cn_bn_workspace_floats", nv.dtype_code(dtype), p, c, nseg, floor=1)[0]


def bn_stats(x, bn, training, nseg=1, count_update=True):
    """(mean, invstd) fp32 [nseg*C] of x = nseg stacked segments of equal rows, each its own
    BN batch (one reference BN call per frame).  Train mode updates bn.running_* once per
    segment, in order (momentum 0.1 each)."""
    p, c = x.shape
    if p % nseg:
        raise ValueError("rows %d not divisible into %d segments" % (p, nseg))
    p //= nseg
    mean = torch.empty((nseg * c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    if training:
        _check_train_rows(p, 1, c)
        ws = _ws(x.dtype, p, c, x.device, nseg)
        nv.call("cn_bn_stats", dtc(x), *_mat(x), p, nseg, c, mean.data_ptr(),
                invstd.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                _momentum(bn), float(bn.eps), ws.data_ptr(), nv.stream())
        if count_update:
            _count_batches(bn, nseg)
    else:
        nv.call("cn_bn_eval_params", bn.running_mean.data_ptr(), bn.running_var.data_ptr(), c,
                float(bn.eps), mean.data_ptr(), invstd.data_ptr(), nv.stream())
        if nseg > 1:
            mean[c:].view(nseg - 1, c).copy_(mean[:c].expand(nseg - 1, c))
            invstd[c:].view(nseg - 1, c).copy_(invstd[:c].expand(nseg - 1, c))
    return mean, invstd


def seg_of(stats, i, c):
    """Statistics of segment i out of bn_stats(..., nseg)."""
    return stats[0][i * c:(i + 1) * c], stats[1][i * c:(i + 1) * c]


def _affine(bn):
    if bn.affine:
        return bn.weight, bn.bias
    return None, None


def relu_mask(p, c, like):
    """Bit-mask buffer for bn_apply(mask=...): [p, c / vec] bytes (vec = channels per 16-B chunk)."""
    vec = 8 if like.dtype == torch.bfloat16 else 4
    return torch.empty((p, c // vec), dtype=torch.uint8, device=like.device)


def _bn_apply_args(x, stats, bn, act, prelu, res, xr, rstats, rbn, nseg):
    """The arguments cn_bn_apply_ex and cn_bn_apply_q8 share, dtype to prelu: each wrapper appends
    its outputs."""
    p, c = x.shape
    g, b = _affine(bn)
    rg, rb = _affine(rbn) if rbn is not None else (None, None)
    return (dtc(x), *_mat(x), p // nseg, nseg, c, stats[0].data_ptr(), stats[1].data_ptr(), nv.ptr(g),
            nv.ptr(b), *_mat(res, 0), *_mat(xr, 0), nv.ptr(rstats[0] if rstats else None),
            nv.ptr(rstats[1] if rstats else None), nv.ptr(rg), nv.ptr(rb), act, nv.ptr(prelu))


def bn_apply(x, stats, bn, act=0, prelu=None, res=None, xr=None, rstats=None, rbn=None, out=None,
             nseg=1, out8=None, qstate=None, mask=None):
    """y = act(bn(x) [+ res] [+ rbn(xr)]) with per-segment statistics ([nseg*C] each); with
    out8 / qstate also an fp8 copy of y (delayed scaling, amax collected into qstate); with mask
    (relu_mask) also y > 0 as bits, which bn_bwd(act=4) takes instead of y.

    The fp8 copy (bf16 only; out8 row stride a multiple of 16) is quantised from the fp32 value of
    the activation BEFORE its rounding to bf16: out8 = e4m3(clamp(t * qstate[1], +-448)) and
    qstate[2] = max |t| with t the fp32 activation, so out8 is not the quantised stored y."""
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device)
    nv.call("cn_bn_apply_ex", *_bn_apply_args(x, stats, bn, act, prelu, res, xr, rstats, rbn, nseg),
            *_mat(out), *_mat(out8, 0), nv.ptr(qstate), nv.ptr(mask),
            mask.stride(0) if mask is not None else 0, nv.stream())
    return out


def bn_apply_q8(x, stats, bn, qstate, act=0, prelu=None, res=None, xr=None, rstats=None, rbn=None,
                out=None, out8=None, nseg=1):
    """bn_apply whose e4m3 image out8 is written under the frozen, read-only qstate
    (cn_bn_apply_q8: no amax, nothing written to qstate); the bf16 output only into a given
    `out`.  Returns (out or None, out8)."""
    if out8 is None:
        out8 = torch.empty(tuple(x.shape), dtype=torch.uint8, device=x.device)
    nv.call("cn_bn_apply_q8", *_bn_apply_args(x, stats, bn, act, prelu, res, xr, rstats, rbn, nseg),
            *_mat(out, 0), *_mat(out8), qstate.data_ptr(), nv.stream())
    return out, out8


def bn_bwd(x, dy, y, stats, bn, act=0, prelu=None, want_dx=True, dx=None, dres=None, dgamma=None,
           dbeta=None, dprelu=None):
    """Train-mode BN backward (+ fused activation mask).  Returns dx, dgamma, dbeta, dprelu
    (dgamma / dbeta / dprelu written into the given buffers if any, e.g. gradient-arena slices).
    act=1 with y=None: the ReLU mask is recomputed from x with the forward's affine (no read of
    the activation; only valid when y = relu(bn(x)) had no residual added).  act=4: y is the
    bit mask bn_apply(mask=...) wrote (1/16 of y's bytes)."""
    p, c = x.shape
    if act == 1 and y is None:
        act = 3
    if dgamma is None:
        dgamma = torch.empty((c,), dtype=torch.float32, device=x.device)
    if dbeta is None:
        dbeta = torch.empty((c,), dtype=torch.float32, device=x.device)
    dpc = torch.empty((c,), dtype=torch.float32, device=x.device) if act == 2 else None
    if want_dx and dx is None:
        dx = torch.empty((p, c), dtype=x.dtype, device=x.device)
    ws = _ws(x.dtype, p, c, x.device)
    g, b = _affine(bn)
    # act 4: y is the bit mask, whose row stride is taken as it is (bytes)
    ym = (y.data_ptr(), y.stride(0)) if act == 4 and y is not None else _mat(y, 0)
    nv.call("cn_bn_bwd", dtc(x), *_mat(x), *_mat(dy), *ym, p, c, stats[0].data_ptr(), stats[1].data_ptr(),
            nv.ptr(g), nv.ptr(b), act, nv.ptr(prelu), dgamma.data_ptr(), dbeta.data_ptr(), nv.ptr(dpc),
            *_mat(dx, 0), *_mat(dres, 0), ws.data_ptr(), nv.stream())
    if dpc is not None:  # per-channel partials -> the single PReLU weight (fixed order)
        if dprelu is None:
            dprelu = torch.empty((1,), dtype=torch.float32, device=x.device)
        nv.call("cn_sum_rows", dpc.data_ptr(), c, 1, dprelu.data_ptr(), nv.stream())
    return dx, dgamma, dbeta, dprelu


def cast_copy(src, dst, accumulate=False):
    nv.call("cn_cast2d", dtc(src), dtc(dst), *_mat(src), src.shape[0], src.shape[1], *_mat(dst),
            int(accumulate), nv.stream())
    return dst
