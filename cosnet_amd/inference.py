"""N-reference inference of test.py (:287-305) and its evaluation (:307-344).

The reference re-encodes the target frame once per reference frame and averages x1 over the
N forwards.  In eval mode every op is per-sample (BN uses running statistics), so encoding
the target once, the N search frames as one batch, and running the co-attention head on the
N-way stack gives the same average (6e-8 in fp32) with 1 + N instead of 2N
encoder passes.
"""
import torch

from . import _native as nv
from . import ops


@torch.no_grad()
def multi_reference_x1(model, target, target_depth, searches, search_depths):
    """target [1,3,H,W], target_depth [1,1,H,W], searches [N,3,H,W], search_depths [N,1,H,W]
    (fp32 NCHW on the GPU) -> mean over the N references of x1, [1,1,H,W] fp32."""
    if model.training:
        raise RuntimeError("multi-reference inference runs in eval mode (test.py:230)")
    if getattr(model, "fp8_static", None) is not None:
        # features_nhwc is the per-module path: it would run bf16 convs without saying so
        raise RuntimeError("multi_reference_x1 does not run static fp8 encoders: use "
                           "segment_sequence (or set_fp8_static(None))")
    if getattr(model, "bn_fold", None) is not None:
        raise RuntimeError("multi_reference_x1 does not run the BN fold: use segment_sequence "
                           "(or set_bn_fold(False))")
    model._set_dtype()
    target, target_depth, searches, search_depths = map(
        model._prep, (target, target_depth, searches, search_depths))
    n = searches.shape[0]
    input_size = tuple(target.shape[2:])
    va, geo1 = model.encoder.features_nhwc(target)
    da, _ = model.depth_encoder.features_nhwc(target_depth)
    vb, geo = model.encoder.features_nhwc(searches)
    db, _ = model.depth_encoder.features_nhwc(search_depths)
    p1 = va.shape[0]
    va_n = torch.empty((n * p1, va.shape[1]), dtype=va.dtype, device=va.device)
    da_n = torch.empty_like(va_n)
    for i in range(n):  # stack the target features N times (one copy kernel each)
        ops.cast_copy(va, va_n[i * p1:(i + 1) * p1])
        ops.cast_copy(da, da_n[i * p1:(i + 1) * p1])
    x1, _ = model.head_nhwc(va_n, vb, da_n, db, geo, input_size)
    out = torch.empty((1, 1) + input_size, dtype=torch.float32, device=x1.device)
    hw = input_size[0] * input_size[1]
    # mean over the N outputs: a fixed-order [N][HW] -> [HW] column reduction scaled by 1/N
    x1 = x1.contiguous()
    nv.call("cn_mean_rows", x1.data_ptr(), n, hw, out.data_ptr(), nv.stream())
    return out


# ---- whole-sequence inference: every frame encoded once, pairs formed by index --------------------
#
# test.py:287-305 forwards each target with N references drawn from the same sequence
# (sbm_rgbd_loader.py:538-579), so over T targets the per-target path encodes (1 + N) T frames of
# which T are distinct.  A FeatureBank holds each frame's features once; the co-attention, gate and
# concat kernels read the frames a pair names in place (cn_coatt_fused_fwd_idx, cn_gate_cat_idx),
# and only the a side -- all test.py uses -- is computed (RGBDSegmentation_RAA.head_a_indexed).

def _as_int_list(x, what):
    if torch.is_tensor(x):
        x = x.tolist()
    try:
        return [int(v) for v in x]
    except TypeError:
        raise ValueError("%s: a flat list of frame indices is expected" % what)


def plan_pairs(n_frames, targets, refs):
    """(ia, ib) int32 CPU tensors of length Tt*N for targets [Tt] and refs [Tt][N] (lists or CPU
    tensors of frame indices into a bank of n_frames): pair t*N + j co-attends targets[t] (a role)
    with refs[t][j] (b role), target-major in reference order.  Self-references and repeated
    references are legal (the reference's sampler draws both)."""
    targets = _as_int_list(targets, "targets")
    if torch.is_tensor(refs):
        if refs.dim() != 2:
            raise ValueError("refs: a [Tt][N] table is expected")
        refs = refs.tolist()
    refs = [_as_int_list(r, "refs[%d]" % i) for i, r in enumerate(refs)]
    if len(refs) != len(targets):
        raise ValueError("refs has %d rows for %d targets" % (len(refs), len(targets)))
    n = len(refs[0]) if refs else 0
    if n < 1:
        raise ValueError("every target needs at least one reference (N >= 1)")
    ia, ib = [], []
    for t, row in zip(targets, refs):
        if len(row) != n:
            raise ValueError("ragged refs: rows of %d and %d references" % (n, len(row)))
        for f in [t] + row:
            if not 0 <= f < n_frames:
                raise ValueError("frame index %d outside the bank of %d frames" % (f, n_frames))
        ia += [t] * n
        ib += row
    return torch.tensor(ia, dtype=torch.int32), torch.tensor(ib, dtype=torch.int32)


class FeatureBank:
    """Per-sequence features, one entry per frame: va / da (the encoders' outputs, V of
    rgbd_segmentation_RAA.py:143-144 / :197-203) and vat / dat (their similarity linears V W^T,
    :158-159 / :211-212), each [T*HW][256] in the model's compute dtype with frame f at rows
    f*HW .. f*HW + HW - 1; geo = (T, h, w) and input_size = (H, W).  coatt = "mxfp8" adds mx / dmx,
    the MX-fp8 images of (vat, va) / (dat, da) (ops.coatt_f8_bank: each frame quantised once, about
    2.9 MB per frame and modality at 473 x 473), and head_a_indexed then runs the fp8 co-attention
    over them; the default "bf16" leaves both None.  partials (reduce_partials: the split head's
    per-frame products, fp32, 3.7 MB per frame and modality at 473 x 473) is None until first asked
    for."""

    COATT = ("bf16", "mxfp8")

    def __init__(self, va, vat, da, dat, geo, input_size, mx=None, dmx=None):
        self.va, self.vat, self.da, self.dat = va, vat, da, dat
        self.geo = tuple(geo)
        self.input_size = tuple(input_size)
        self.mx, self.dmx = mx, dmx
        self.partials = None

    @property
    def n_frames(self):
        return self.geo[0]

    @torch.no_grad()
    def reduce_partials(self, model, frame_chunk=8):
        """(ua, uda), fp32 [T*HW][256]: the pass-through half of each modality's reduce conv over
        the bank's frames, conv_fwd_partial(va, W[..., C:]) (cosnet_amd/head_split.py) -- the fp32
        accumulator, unrounded, which head_a_indexed(split=True) adds per pair through its map.
        Runs in chunks of frame_chunk whole frames (a frame's rows do not depend on the chunking);
        computed on first use and kept on the bank."""
        if self.partials is not None:
            return self.partials
        hs = getattr(model, "head_split", None)
        if hs is None:
            raise RuntimeError("reduce_partials: model.set_head_split() first")
        if frame_chunk < 1:
            raise ValueError("reduce_partials: frame_chunk >= 1 is expected")
        from .head_split import reduce_sides
        t, h, w = self.geo
        hw = h * w
        outs = []
        for v, (reduce, _) in zip((self.va, self.da), reduce_sides(model)):
            _, wv = hs.halves(reduce, v.dtype)
            cout = reduce.weight.shape[0]
            u = torch.empty((t * hw, cout), dtype=torch.float32, device=v.device)
            for f0 in range(0, t, frame_chunk):
                f1 = min(t, f0 + frame_chunk)
                ops.conv_fwd_partial(v[f0 * hw:f1 * hw], f1 - f0, h, w, wv, cout, 3, 1, 1, 1,
                                     out=u[f0 * hw:f1 * hw])
            outs.append(u)
        self.partials = tuple(outs)
        return self.partials

    @staticmethod
    def _similarity(feats, linear):
        from .functions import WCACHE
        c = feats.shape[1]
        wf, _ = WCACHE.get(linear.weight, feats.dtype, need_t=False)
        return ops.gemm(feats, wf, feats.shape[0], c, c, lda=ops.ld(feats), ldb=c)

    @classmethod
    @torch.no_grad()
    def from_features(cls, model, va, da, geo, input_size, coatt="bf16"):
        """The bank of given encoder features va / da [T*HW][C] (geo = (T, h, w))."""
        t, h, w = geo
        if coatt not in cls.COATT:
            raise ValueError("coatt: one of %s is expected, not %r" % (cls.COATT, coatt))
        if va.shape != da.shape or va.shape[0] != t * h * w or va.dtype != model.compute_dtype:
            raise ValueError("from_features: va / da must be [T*h*w][C] in the model's compute dtype")
        if coatt == "mxfp8" and (va.dtype != torch.bfloat16 or va.shape[1] != 256):
            raise ValueError("coatt='mxfp8' needs the bf16 compute dtype and 256 feature channels")
        vat = cls._similarity(va, model.rgb_similarity_weights)
        dat = cls._similarity(da, model.depth_similarity_weights)
        mx = dmx = None
        if coatt == "mxfp8":
            mx = ops.coatt_f8_bank(vat, va, t, h * w)
            dmx = ops.coatt_f8_bank(dat, da, t, h * w)
        return cls(va, vat, da, dat, geo, input_size, mx, dmx)

    @classmethod
    @torch.no_grad()
    def encode(cls, model, rgbs, depths, encode_chunk=8, coatt="bf16"):
        """rgbs [T,3,H,W], depths [T,1,H,W] (fp32 NCHW on the GPU): both encoders over chunks of
        encode_chunk frames, then the two similarity linears (and, coatt = "mxfp8", the MX images),
        once per frame.  On a model with static fp8 set (model.set_fp8_static) the encoders run
        fp8_infer.encode_frames_static: e4m3 conv GEMMs on frozen scales; the bank stays bf16.  On
        a model with the BN fold set (model.set_bn_fold) they run bn_fold.encode_frames_folded."""
        if model.training:
            raise RuntimeError("FeatureBank.encode runs in eval mode (test.py:230)")
        if coatt not in cls.COATT:
            raise ValueError("coatt: one of %s is expected, not %r" % (cls.COATT, coatt))
        if coatt == "mxfp8" and model.compute_dtype != torch.bfloat16:   # before any encoder pass
            raise ValueError("coatt='mxfp8' needs the bf16 compute dtype")
        if rgbs.shape[0] != depths.shape[0] or rgbs.shape[0] < 1 or encode_chunk < 1:
            raise ValueError("encode: T >= 1 frames of rgb and depth and encode_chunk >= 1 are expected")
        static = getattr(model, "fp8_static", None) is not None
        if static and model.compute_dtype != torch.bfloat16:
            raise ValueError("static fp8 encoders need the bf16 compute dtype")
        model._set_dtype()
        rgbs, depths = model._prep(rgbs), model._prep(depths)
        t = rgbs.shape[0]
        va = da = None
        if static:   # e4m3 conv GEMMs on frozen scales (cosnet_amd/fp8_infer.py); the bank stays bf16
            from .fp8_infer import encode_frames_static
            feats = lambda enc, x: encode_frames_static(enc, x)
        elif getattr(model, "bn_fold", None) is not None:   # one launch per conv + eval BN pair
            from .bn_fold import encode_frames_folded
            feats = lambda enc, x: encode_frames_folded(enc, x)
        else:
            feats = lambda enc, x: enc.features_nhwc(x)
        for f0 in range(0, t, encode_chunk):
            f1 = min(t, f0 + encode_chunk)
            v, (_, h, w) = feats(model.encoder, rgbs[f0:f1])
            d, dgeo = feats(model.depth_encoder, depths[f0:f1])
            if tuple(dgeo[1:]) != (h, w):
                raise RuntimeError("RGB and depth feature maps differ: %s vs %s" % ((h, w), dgeo[1:]))
            if va is None:
                if f1 == t:        # one chunk: its outputs are the bank
                    va, da = v, d
                    break
                va = torch.empty((t * h * w, v.shape[1]), dtype=v.dtype, device=v.device)
                da = torch.empty_like(va)
            ops.cast_copy(v, va[f0 * h * w:f1 * h * w])
            ops.cast_copy(d, da[f0 * h * w:f1 * h * w])
        return cls.from_features(model, va, da, (t, h, w), tuple(rgbs.shape[2:]), coatt)


@torch.no_grad()
def segment_sequence(model, rgbs, depths, refs, targets=None, encode_chunk=8, pair_chunk=10,
                     coatt="bf16", head="cat"):
    """rgbs [T,3,H,W], depths [T,1,H,W] (fp32 NCHW on the GPU), refs [Tt][N] and targets [Tt]
    (default: every frame in order) frame indices -> [Tt,1,H,W] fp32 whose row t is
    multi_reference_x1(model, rgbs[t], depths[t], rgbs[refs[t]], depths[refs[t]]) up to rounding:
    every frame is encoded once and the a-side head runs over chunks of whole targets of about
    pair_chunk pairs.  coatt = "mxfp8" (bf16 models): the co-attention runs on MX-fp8 images of
    the bank (FeatureBank); "bf16" (default): the bf16 indexed kernel.  head = "split"
    (model.set_head_split()): the reduce convs run split by input-channel half, the pass-through
    half once per frame (cosnet_amd/head_split.py); "cat" (default): over the concat, per pair."""
    if head not in ("cat", "split"):
        raise ValueError("head: 'cat' or 'split' is expected, not %r" % (head,))
    t = rgbs.shape[0]
    if targets is None:
        targets = list(range(t))
    ia, ib = plan_pairs(t, targets, refs)
    nt = len(targets)
    n = ia.shape[0] // nt
    bank = FeatureBank.encode(model, rgbs, depths, encode_chunk, coatt)
    hw = bank.input_size[0] * bank.input_size[1]
    out = torch.empty((nt, 1) + bank.input_size, dtype=torch.float32, device=bank.va.device)
    step = max(1, int(pair_chunk) // n)   # whole targets per head call
    for t0 in range(0, nt, step):
        t1 = min(nt, t0 + step)
        x1 = model.head_a_indexed(bank, ia[t0 * n:t1 * n], ib[t0 * n:t1 * n], split=head == "split")
        ops.mean_groups(x1.view((t1 - t0) * n, hw), t1 - t0, n, out=out[t0:t1].view(t1 - t0, hw))
    return out


@torch.no_grad()
def resize_linear(x, out_hw):
    """cv2.resize(..., INTER_LINEAR) of a float map (half-pixel centres, no antialias), which is
    bilinear with align_corners=False: the upsample kernel without the sigmoid."""
    n, c, h, w = x.shape
    assert c == 1
    H, W = out_hw
    if (H, W) == (h, w):
        return x
    out = torch.empty((n, 1, H, W), dtype=torch.float32, device=x.device)
    src = x.contiguous()
    nv.call("cn_upsample_sigmoid", src.data_ptr(), n, h, w, H, W, 0, out.data_ptr(), nv.stream())
    return out


def masks_uint8(x):
    """(output * 255).astype(np.uint8) of test.py:317 (truncation toward zero)."""
    return (x.detach().float().cpu().numpy() * 255).astype("uint8")


@torch.no_grad()
def soft_iou(x, gt):
    """GPU quantisation + soft-J of test.py:317 / evaluation.py:3-22 (HIP kernel cn_soft_iou).

    x: [n,1,H,W] (or [n,H,W]) fp32 in [0,1] on the GPU; gt: [n,H,W] {0,1} (any integer / bool /
    float dtype holding 0/1; converted to uint8 like the reference's astype).
    Returns (masks [n,H,W] uint8 on the GPU, iou [n] float64 on the GPU, counts [n,4] int64 =
    (sum p&g, sum p|g, nonzero p, nonzero g)).  Bit-exact with evaluation.compute_iou on the
    host masks."""
    n = x.shape[0]
    hw = x.shape[-2] * x.shape[-1]
    if x.dtype != torch.float32 or not x.is_cuda:
        raise RuntimeError("soft_iou: x must be fp32 on the GPU")
    if gt.shape[0] != n or gt.shape[-2] * gt.shape[-1] != hw:
        raise RuntimeError("soft_iou: gt %s does not match x %s" % (tuple(gt.shape), tuple(x.shape)))
    x = x.contiguous()
    g = gt.to(device=x.device, dtype=torch.uint8).contiguous()
    masks = torch.empty((n,) + tuple(x.shape[-2:]), dtype=torch.uint8, device=x.device)
    iou = torch.empty((n,), dtype=torch.float64, device=x.device)
    counts = torch.empty((n, 4), dtype=torch.int64, device=x.device)
    nv.call("cn_soft_iou", x.data_ptr(), g.data_ptr(), n, hw, masks.data_ptr(), iou.data_ptr(),
            counts.data_ptr(), nv.stream())
    return masks, iou, counts
