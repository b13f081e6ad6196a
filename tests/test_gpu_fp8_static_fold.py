"""Eval-mode BatchNorm folded into the static-scale fp8 encoder convs (cosnet_amd/fp8_infer.py
bottleneck_static_folded / aspp_static_folded, model.set_fp8_static(calibration, fold_bn=True),
test.py --feature-bank --dtype fp8 --fp8-fold-bn) at the 65 x 81 input with 4 frames, as
tests/test_gpu_fp8_static.py.

* wiring, bitwise: the folded block functions against the same launches written out here with
  ops.conv_fwd_fp8_affine on state copies (cn_conv_fwd_fp8_affine itself is pinned bitwise by
  tests/test_gpu_conv_fp8_affine.py);
* launch census: one conv launch per conv + BN pair, no BN launch, no unfolded fp8 conv;
* frozen and stateless; load_state_dict is followed;
* accuracy against the UNFOLDED static path's error, truth = the fp32 default path;
* refusals, switching, the command line.
"""
import os

import pytest
import torch

from cosnet_amd import encoder_fn as E
from cosnet_amd import fp8_infer as FI
from cosnet_amd import ops
from cosnet_amd.inference import FeatureBank, multi_reference_x1, segment_sequence

from test_gpu_fp8_static import (HW, SIZE, _run_cli, bf16_model, calib20, cli_env, four_frames,  # noqa: F401
                                 fp32_model, make_model, tables)                                  # (fixtures)

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
PAIRS = {"encoder": 110, "depth_encoder": 59}     # conv + BN pairs of one pass


@pytest.fixture(scope="module")
def model(cuda, calib20):
    """One bf16 model and its two static states on one calibration: unfolded and folded."""
    m = make_model(cuda, bf)
    plain = m.set_fp8_static(calib20).fp8_static
    fold = m.set_fp8_static(None).set_fp8_static(calib20, fold_bn=True).fp8_static
    m.set_fp8_static(None)
    return m, plain, fold


@pytest.fixture
def folded(model, request):
    m, _, fold = model
    m.set_fp8_static(fold)
    request.addfinalizer(lambda: m.set_fp8_static(None))
    return m


def bits_equal(a, b):
    v = torch.int16 if a.dtype == bf else torch.int32 if a.dtype == torch.float32 else a.dtype
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


# ---- wiring, bitwise ----------------------------------------------------------------------------------
def _conv8(S, x8, n, h, w, conv, bn, cout, k, stride, pad, dil, x_state, **kw):
    w8, ws = S.w8(conv.weight)
    sc, sf = ops.bn_fold_table(bn)                  # a table of its own, not the state's
    return ops.conv_fwd_fp8_affine(x8, n, h, w, w8, cout, k, stride, pad, dil, x_state.clone(), ws.clone(),
                                   sc, sf, **kw)


@pytest.mark.parametrize("index", [1, 0])
def test_folded_bottleneck_is_its_launches_written_out(cuda, folded, index):
    """layer2[1] (identity) and layer2[0] (downsample, stride 2) on a [2 * 99]-row input."""
    m = folded
    enc = m.encoder
    S = enc._cn_fp8_static
    assert S.fold is not None
    blk = enc.backbone.layer2[index]
    name, nxt = "backbone.layer2.%d" % index, "backbone.layer2.%d.x" % (index + 1)
    cin, planes = blk.conv1.weight.shape[1], blk.conv1.weight.shape[0]
    s, d = blk.stride, blk.dilation
    assert (blk.downsample is not None) == (index == 0) and s == (2 if index == 0 else 1)
    n, h, w = geo = (2, 9, 11)
    g = torch.Generator().manual_seed(60 + index)
    x = (torch.rand((2 * HW, cin), generator=g) * 2.0).to(bf).to(cuda)
    st = lambda nm: S.st(nm).clone()
    with torch.no_grad():
        m._set_dtype()
        x8 = ops.fp8_quant_static(x, S.st(name + ".x"))
        y, y8, ogeo = FI.bottleneck_static_folded(blk, x, x8, geo, S, S.st(nxt))
        r1, y18, oh, ow = _conv8(S, x8, n, h, w, blk.conv1, blk.bn1, planes, 1, s, 0, 1, st(name + ".x"),
                                 act=1, out_state=st(name + ".y1"), want_y=False)
        r2, y28, _, _ = _conv8(S, y18, n, oh, ow, blk.conv2, blk.bn2, planes, 3, 1, d, d, st(name + ".y1"),
                               act=1, out_state=st(name + ".y2"), want_y=False)
        assert r1 is None and r2 is None            # y1 / y2 exist as e4m3 only
        res = x
        if index == 0:
            res, none8, _, _ = _conv8(S, x8, n, h, w, blk.downsample[0], blk.downsample[1], 4 * planes, 1, s, 0, 1,
                                      st(name + ".x"), act=0)
            assert none8 is None and res.dtype == bf
            assert (res.float() < 0).any(), "rd carries no activation: negative values survive"
        ry, r8, _, _ = _conv8(S, y28, n, oh, ow, blk.conv3, blk.bn3, 4 * planes, 1, 1, 0, 1, st(name + ".y2"),
                              act=1, res=res, out_state=st(nxt))
    torch.cuda.synchronize()
    assert ogeo == (n, oh, ow) and y.shape == (n * oh * ow, 4 * planes) and y8.dtype == torch.uint8
    assert torch.isfinite(ry.float()).all() and ry.float().abs().max() > 0 and len(torch.unique(r8)) > 16
    assert bits_equal(y, ry) and bits_equal(y8, r8)


def test_folded_aspp_is_its_launches_written_out(cuda, folded):
    m = folded
    enc = m.depth_encoder                           # its dilations differ from the RGB encoder's
    S, mod = enc._cn_fp8_static, enc.aspp
    n, h, w = geo = (2, 9, 11)
    P = n * h * w
    g = torch.Generator().manual_seed(77)
    x = (torch.rand((P, 2048), generator=g) * 2.0).to(bf).to(cuda)
    sx, sc = S.st("aspp.x").clone(), S.st("aspp.cat").clone()
    with torch.no_grad():
        m._set_dtype()
        x8 = ops.fp8_quant_static(x, S.st("aspp.x"))
        got = FI.aspp_static_folded(mod, x, x8, geo, S)
        pool = torch.empty((n, 2048), dtype=bf, device=cuda)
        ops.avgpool(x, n, h * w, 1.0 / (h * w), pool)
        wcf, _ = ops.WCACHE.get(mod.conv.weight, bf)
        yp, _, _ = ops.conv_fwd_affine(pool, n, 1, 1, wcf, 512, 1, 1, 0, 1, *ops.bn_fold_table(mod.bn_x), act=1,
                                       bias=mod.conv.bias)
        cat8 = torch.full((P, 2560), 0x7F, dtype=torch.uint8, device=cuda)
        ops.bcast_rows_u8(ops.fp8_quant_static(yp, sc), n, h * w, cat8[:, :512])
        for bi, (cm, bnm, k, dd) in enumerate(E.aspp_branches(mod)):
            r, s8, _, _ = _conv8(S, x8, n, h, w, cm, bnm, 512, k, 1, dd, max(dd, 1), sx, act=1, bias=cm.bias,
                                 out8=cat8[:, 512 * (bi + 1):512 * (bi + 2)], out_state=sc, want_y=False)
            assert r is None and s8.data_ptr() == cat8[:, 512 * (bi + 1):].data_ptr()   # written in place
        ref, none8, _, _ = _conv8(S, cat8, n, h, w, mod.bottleneck, mod.bn, 256, 3, 1, 1, 1, sc, act=2,
                                  prelu=mod.prelu.weight, bias=mod.bottleneck.bias)
    torch.cuda.synchronize()
    assert none8 is None and got.shape == (P, 256) and got.dtype == bf
    assert torch.isfinite(ref.float()).all() and (ref.float() < 0).any() and not (cat8 == 0x7F).all(1).any()
    assert bits_equal(got, ref)


# ---- launch census ------------------------------------------------------------------------------------
def test_one_launch_per_conv_bn_pair(cuda, folded, monkeypatch):
    m = folded
    rgbs, deps = four_frames(cuda, 21)
    count = {}

    def wrap(name):
        real = getattr(ops, name)

        def f(*a, **k):
            count[name] = count.get(name, 0) + 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, f)

    for name in ("conv_fwd_fp8_affine", "conv_fwd_affine", "conv_fwd_fp8", "conv_fwd", "bn_stats", "bn_apply",
                 "bn_apply_q8", "conv_fwd_bn"):
        wrap(name)
    with torch.no_grad():
        m._set_dtype()
        for key, x in (("encoder", rgbs), ("depth_encoder", deps)):
            count.clear()
            enc = getattr(m, key)
            feats, geo = FI.encode_frames_static(enc, m._prep(x))
            torch.cuda.synchronize()
            assert geo == (4, 9, 11) and torch.isfinite(feats.float()).all()
            n_bn = sum(1 for mod in enc.modules() if isinstance(mod, torch.nn.BatchNorm2d))
            assert n_bn == PAIRS[key] == len(enc._cn_fp8_static.fold)
            # the stem and the ASPP's pooled 1x1 conv are bf16 launches, every other pair is fp8
            assert count == {"conv_fwd_fp8_affine": PAIRS[key] - 2, "conv_fwd_affine": 2}, (key, count)


# ---- frozen and stateless -----------------------------------------------------------------------------
def test_frozen_stateless_and_follows_load_state_dict(cuda, calib20):
    m = make_model(cuda, bf).set_fp8_static(calib20, fold_bn=True)      # its own model: the state changes
    X, other = four_frames(cuda, 21), four_frames(cuda, 22)
    fold_tabs = lambda: [t.clone() for S in m.fp8_static.encoders.values() for t in S.fold._tab.values()]
    enc = lambda: FeatureBank.encode(m, *X)
    same = lambda a, b: all(bits_equal(getattr(a, k), getattr(b, k)) for k in ("va", "da", "vat", "dat"))
    before, fbefore = [t.clone() for t in tables(m)], fold_tabs()
    a = enc()
    keep = {k: getattr(a, k).clone() for k in ("va", "da")}
    FeatureBank.encode(m, other[0] * 10, other[1] * 10)                 # every amax would move
    b = enc()
    torch.cuda.synchronize()
    assert a.va.dtype == bf and a.va.shape == (4 * HW, 256) and torch.isfinite(a.va.float()).all()
    assert bits_equal(keep["va"], b.va) and bits_equal(keep["da"], b.da)
    for x, y in zip(before + fbefore, tables(m) + fold_tabs()):
        assert bits_equal(x, y)
    # other running statistics: FoldTables' version rule rebuilds the tables and the features follow
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict({k: (v * 1.5 if k.endswith("running_var") else v) for k, v in sd.items()})
    c = enc()
    assert not bits_equal(c.va, keep["va"]) and not bits_equal(c.da, keep["da"])
    fresh = m.set_fp8_static(None).set_fp8_static(calib20, fold_bn=True)   # tables built from the new statistics
    assert same(c, FeatureBank.encode(fresh, *X))
    m.load_state_dict(sd)
    d = enc()
    assert bits_equal(d.va, keep["va"]) and bits_equal(d.da, keep["da"])


# ---- accuracy against the unfolded static path ---------------------------------------------------------
@pytest.mark.parametrize("seed", [21, 22, 23])
def test_folded_is_no_worse_than_unfolded_against_fp32(cuda, model, fp32_model, seed):
    """mean |x1 - x1_fp32| of segment_sequence (1 target x 3 references) with fold_bn=True is at
    most 1.5 x that with fold_bn=False on the same calibration.  The folded path rounds once per
    conv + BN pair where the unfolded one rounds the raw conv output to bf16 first, so it should
    not be worse; 1.5 is the margin tests/test_gpu_bn_fold.py uses for the same comparison on
    this rounding-amplifying seeded network."""
    m, plain, fold = model
    rgbs, deps = four_frames(cuda, seed)
    run = lambda mm: segment_sequence(mm, rgbs, deps, [[1, 2, 3]], targets=[0]).double().cpu()
    truth = run(fp32_model)
    errs = {}
    for tag, st in (("unfolded", plain), ("folded", fold)):
        m.set_fp8_static(st)
        try:
            x1 = run(m)
        finally:
            m.set_fp8_static(None)
        assert x1.shape == (1, 1) + SIZE and torch.isfinite(x1).all() and x1.min() >= 0 and x1.max() <= 1
        errs[tag] = (x1 - truth).abs().mean().item()
    print("seed %d static fp8, mean |x1 - x1_fp32|: unfolded %.4e, folded %.4e, ratio %.3f (bound 1.5)"
          % (seed, errs["unfolded"], errs["folded"], errs["folded"] / errs["unfolded"]))
    assert errs["unfolded"] > 0 and errs["folded"] <= 1.5 * errs["unfolded"], (seed, errs)


# ---- refusals and switching -----------------------------------------------------------------------------
def test_refusals_and_switching(cuda, model, bf16_model, calib20):
    m, plain, fold = model
    rgbs, deps = four_frames(cuda, 21)
    assert plain.head is None and not plain.fold_bn and all(S.fold is None for S in plain.encoders.values())
    assert fold.fold_bn and len(fold.head) == 2 and [len(fold.encoders[k].fold) for k in FI.ENCODERS] == [110, 59]
    with torch.no_grad():
        default = FeatureBank.encode(m, rgbs, deps)
    m.set_fp8_static(fold)
    try:
        assert m.fp8_static is fold and m.bn_fold is None
        assert m.encoder._cn_fp8_static is fold.encoders["encoder"] and getattr(m.encoder, "_cn_bn_fold", None) is None
        with pytest.raises(RuntimeError, match="set_fp8_static"):
            m.set_bn_fold()
        with pytest.raises(RuntimeError):
            m.set_fp8(True)
        assert m.fp8 is None and m.bn_fold is None
        with pytest.raises(RuntimeError, match="segment_sequence"):
            multi_reference_x1(m, rgbs[:1], deps[:1], rgbs[1:], deps[1:])
        with pytest.raises(RuntimeError):                     # grad enabled
            FI.encode_frames_static(m.encoder, rgbs)
        with pytest.raises(RuntimeError):                     # the pair forward
            m(rgbs[:1], rgbs[1:2], deps[:1], deps[1:2])
        m.train()
        try:
            with pytest.raises(RuntimeError):
                FeatureBank.encode(m, rgbs, deps)
            with torch.no_grad(), pytest.raises(RuntimeError):
                FI.encode_frames_static(m.encoder, rgbs)
            with pytest.raises(RuntimeError, match="eval"):
                FI.Fp8Static(m, calib20, fold_bn=True)        # the fold uses running statistics
        finally:
            m.eval()
        with pytest.raises(ValueError):                       # a state built for another model
            bf16_model.set_fp8_static(fold)
        with torch.no_grad():
            on = FeatureBank.encode(m, rgbs, deps)
            assert m.head_a_indexed(on, [0, 0], [1, 3]).shape == (2, 1) + SIZE
        # a built state handed back keeps the fold state it was built with, whatever fold_bn says
        assert m.set_fp8_static(plain, fold_bn=True).fp8_static is plain and m.encoder._cn_fp8_static.fold is None
        assert m.set_fp8_static(fold).fp8_static is fold and m.encoder._cn_fp8_static.fold is not None
    finally:
        m.set_fp8_static(None)
    assert m.fp8_static is None and m.encoder._cn_fp8_static is None and m.depth_encoder._cn_fp8_static is None
    with torch.no_grad():
        off = FeatureBank.encode(m, rgbs, deps)               # the default path again
        m.set_fp8_static(fold)
        try:
            again = FeatureBank.encode(m, rgbs, deps)         # the built state switches it back on
        finally:
            m.set_fp8_static(None)
    torch.cuda.synchronize()
    assert bits_equal(off.va, default.va) and bits_equal(off.da, default.da)
    assert bits_equal(again.va, on.va) and bits_equal(again.da, on.da)
    assert not bits_equal(on.va, default.va)
    m.set_bn_fold()                                           # the existing refusal, the other way round
    try:
        with pytest.raises(RuntimeError, match="set_bn_fold"):
            m.set_fp8_static(calib20, fold_bn=True)
    finally:
        m.set_bn_fold(False)


# ---- test.py --feature-bank --dtype fp8 --fp8-fold-bn -------------------------------------------------------
def test_cli_fp8_fold_bn_is_repeatable(cuda, cli_env):
    F = os.path.join(cli_env[0], "calibration_fold.json")
    plain = _run_cli(cli_env, "fp8_plain", ["--dtype", "fp8", "--fp8-calibration", F])
    assert os.path.exists(F)
    made = open(F, "rb").read()
    a = _run_cli(cli_env, "fp8_fold_a", ["--dtype", "fp8", "--fp8-calibration", F, "--fp8-fold-bn"])
    b = _run_cli(cli_env, "fp8_fold_b", ["--dtype", "fp8", "--fp8-calibration", F, "--fp8-fold-bn"])
    assert open(F, "rb").read() == made
    assert len(a[0]) == 13 and plain[0] == a[0] == b[0] and len(a[3]) == 13
    assert a[3] == b[3], "PNG bytes differ between two runs on one calibration file"
    assert a[1] == b[1] and a[2] == b[2]
    print("sbmrgbd 13 frames: final IOU static fp8 bank %s, with --fp8-fold-bn %s; max per-frame |d| %.2e" % (
        plain[2], a[2], max(abs(float(x) - float(y)) for x, y in zip(plain[1], a[1]))))
