"""Static-scale fp8 encoders for whole-sequence inference (cosnet_amd/fp8_infer.py,
RGBDSegmentation_RAA.set_fp8_static, FeatureBank.encode, test.py --dtype fp8) at the 65 x 81 input
(map 9 x 11, HW = 99: even one frame is above the 64-row threshold in every layer).

* calibration is a function of the frame set (chunking, order, save / load);
* history independence: a frame's features do not depend on what was encoded before it, and no
  state table changes -- the property delayed scaling lacks;
* wiring, exact: the static bottleneck step is bitwise the composition of the existing kernels
  (delayed-mode quantise on state copies, cn_conv_fwd_fp8, cn_bn_apply_fp8) under the same scales;
* accuracy of the features against the fp32 path, bounded by 32 x the bf16 path's own error;
* end to end, refusals, test.py.
"""
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import golden
import cosnet_amd as C
from cosnet_amd import encoder_fn as E
from cosnet_amd import fp8_infer as FI
from cosnet_amd import ops
from cosnet_amd.inference import FeatureBank, multi_reference_x1, segment_sequence
from cosnet_amd.init_recipe import recipe_state_dict, synthetic_inputs

pytestmark = pytest.mark.gpu

SIZE, HW, N = (65, 81), 99, 3

_SD = {}


def state_dict(calib_name, like):
    """The seeded recipe plus a fixture's calibrated BN statistics (computed once per fixture)."""
    if calib_name not in _SD:
        sd = recipe_state_dict(like.state_dict())
        calib = golden(calib_name)
        for k in calib.files:
            sd[k[len("calib/"):]] = torch.from_numpy(calib[k])
        _SD[calib_name] = sd
    return _SD[calib_name]


def make_model(cuda, dtype, calib_name="bn_calibration.npz"):
    m = C.build_model(dtype)
    m.load_state_dict(state_dict(calib_name, m))
    return m.to(cuda).eval() if cuda is not None else m


def four_frames(cuda, seed):
    """1 target + 3 references, distinct frames."""
    ra, rb, da, db, _, _ = synthetic_inputs(N, SIZE[0], SIZE[1], seed=seed, correlated=False)
    return torch.cat([ra[:1], rb]).to(cuda), torch.cat([da[:1], db]).to(cuda)


@pytest.fixture(scope="module")
def bf16_model(cuda):
    return make_model(cuda, torch.bfloat16)


@pytest.fixture(scope="module")
def fp32_model(cuda):
    return make_model(cuda, torch.float32)


@pytest.fixture(scope="module")
def calib20(cuda, bf16_model):
    """Calibrated on the frames of seed 20: other frames than any test below encodes."""
    return FI.calibrate(bf16_model, *four_frames(cuda, 20))


@pytest.fixture(scope="module")
def static_model(cuda, calib20):
    return make_model(cuda, torch.bfloat16).set_fp8_static(calib20)


def f32_bits(v):
    return struct.pack("<f", v)


def tables(m):
    return [m.fp8_static.encoders[k].states for k in FI.ENCODERS]


# ---- 4. calibration ----------------------------------------------------------------------------------
def test_calibration_is_a_function_of_the_frame_set(cuda, bf16_model, tmp_path):
    m = bf16_model
    rgbs, deps = four_frames(cuda, 20)
    c1 = FI.calibrate(m, rgbs, deps, encode_chunk=1)
    c4 = FI.calibrate(m, rgbs, deps, encode_chunk=4)
    cr = FI.calibrate(m, rgbs.flip(0).contiguous(), deps.flip(0).contiguous(), encode_chunk=3)
    for k in FI.ENCODERS:
        assert list(c1.amax[k]) == FI.state_names(getattr(m, k))
        n_blocks = sum(len(l) for l in (getattr(m, k).backbone.layer1, getattr(m, k).backbone.layer2,
                                        getattr(m, k).backbone.layer3, getattr(m, k).backbone.layer4))
        assert len(c1.amax[k]) == 3 * n_blocks + 2
        for n in c1.amax[k]:
            a = c1.amax[k][n]
            assert a > 0 and np.float32(a) == a, (k, n, a)                  # an fp32 value, exactly
            assert f32_bits(a) == f32_bits(c4.amax[k][n]) == f32_bits(cr.amax[k][n]), (k, n)
    assert c1 == c4 == cr
    with torch.no_grad():
        m._set_dtype()
        z, zgeo = m.encoder.backbone.forward_nhwc(m._prep(rgbs))
    assert c4.amax["encoder"]["aspp.x"] == z.float().abs().max().item()
    # the tensors the walk takes from the forward's records: a block with a downsample, one
    # without, and the ASPP's concat, against the block functions run here.  Exact: the amax is an
    # integer atomic max on the float bits and eval-mode BN makes every tensor independent of chunking
    enc, amax = m.encoder, c4.amax["encoder"]
    with torch.no_grad(), E.no_fp8():
        x, geo = E.stem_fwd(enc.backbone, (m._prep(rgbs),), 1, torch.bfloat16, None)
        for i in (0, 1):
            rec = []
            x, geo = E.bottleneck_fwd(enc.backbone.layer1[i], x, geo, 1, rec)
            assert (enc.backbone.layer1[i].downsample is not None) == (i == 0)
            for f in ("y1", "y2"):
                assert amax["backbone.layer1.%d.%s" % (i, f)] == float(getattr(rec[0], f).float().abs().max())
        rec = []
        E.aspp_fwd(enc.aspp, z, zgeo, 1, rec)
        assert zgeo == (4, 9, 11)
        assert amax["aspp.cat"] == float(rec[0].cat.float().abs().max())
    # the tables built from them
    ms = make_model(cuda, torch.bfloat16)
    t1 = [t.clone() for t in tables(ms.set_fp8_static(c1))]
    t2 = tables(ms.set_fp8_static(cr))
    torch.cuda.synchronize()
    for k, a, b in zip(FI.ENCODERS, t1, t2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert (a[:, 2] == 0).all() and (a[:, 3] == 448).all()
        am = torch.tensor(list(c1.amax[k].values()), dtype=torch.float64)
        a = a.double().cpu()            # scale = amax * margin / 448 and its inverse, in fp32
        assert ((a[:, 0] - am / 448).abs() <= 2.0 ** -23 * am / 448).all()
        assert ((a[:, 1] - 1 / a[:, 0]).abs() <= 2.0 ** -23 / a[:, 0]).all()
    # save / load, bit for bit
    path = str(tmp_path / "calib.json")
    c1.save(path)
    back = FI.Fp8Calibration.load(path)
    assert back == c1 and back.margin == 1.0 and back.version == FI.FORMAT_VERSION
    for k in FI.ENCODERS:
        assert list(back.amax[k]) != [] and all(
            f32_bits(back.amax[k][n]) == f32_bits(c1.amax[k][n]) for n in c1.amax[k])


# ---- 5. history independence ---------------------------------------------------------------------------
def test_features_do_not_depend_on_what_was_encoded_before(cuda, static_model):
    m = static_model
    X = four_frames(cuda, 21)
    other = four_frames(cuda, 22)
    before = [t.clone() for t in tables(m)]
    b1 = FeatureBank.encode(m, *X)
    va1, da1 = b1.va.clone(), b1.da.clone()
    FeatureBank.encode(m, other[0] * 10, other[1] * 10)      # every amax would move
    b2 = FeatureBank.encode(m, *X)
    torch.cuda.synchronize()
    assert b1.va.dtype == torch.bfloat16 and b1.va.shape == (4 * HW, 256) and b1.geo == (4, 9, 11)
    assert torch.isfinite(va1.float()).all() and torch.isfinite(da1.float()).all()
    assert torch.equal(va1.view(torch.int16), b2.va.view(torch.int16))
    assert torch.equal(da1.view(torch.int16), b2.da.view(torch.int16))
    for a, b in zip(before, tables(m)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 6. wiring -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [1, 0])
def test_static_bottleneck_is_the_composition_of_the_existing_kernels(cuda, static_model, index):
    """layer2[1] (identity) and layer2[0] (downsample, stride 2) on a [2*99]-row input."""
    m = static_model
    enc = m.encoder
    S = enc._cn_fp8_static
    blk = enc.backbone.layer2[index]
    nxt = "backbone.layer2.%d.x" % (index + 1)
    name = "backbone.layer2.%d" % index
    cin = blk.conv1.weight.shape[1]
    planes = blk.conv1.weight.shape[0]
    s, d = blk.stride, blk.dilation
    assert (blk.downsample is not None) == (index == 0) and s == (2 if index == 0 else 1)
    geo = (2, 9, 11)
    n, h, w = geo
    g = torch.Generator().manual_seed(60 + index)
    x = (torch.rand((2 * HW, cin), generator=g) * 2.0).to(torch.bfloat16).to(cuda)
    with torch.no_grad():
        m._set_dtype()
        y, y8, ogeo = FI.bottleneck_static(blk, x, ops.fp8_quant_static(x, S.st(name + ".x")), geo, S, S.st(nxt))
        # the existing kernels under the same scales, every state a copy
        cp = lambda nm: S.st(nm).clone()
        ev = lambda c, bn: ops.bn_stats(c, bn, False)
        sx, s1, s2, so = cp(name + ".x"), cp(name + ".y1"), cp(name + ".y2"), cp(nxt)
        x8 = ops.fp8_quant(x, sx, ops.FP8_DELAYED)
        c1, oh, ow = ops.conv_fwd_fp8(x8, n, h, w, S.w8(blk.conv1.weight)[0], planes, 1, s, 0, 1,
                                      S.st(name + ".x"), S.w8(blk.conv1.weight)[1])
        y18 = torch.empty(tuple(c1.shape), dtype=torch.uint8, device=cuda)
        ops.bn_apply(c1, ev(c1, blk.bn1), blk.bn1, act=1, out8=y18, qstate=s1)
        c2, _, _ = ops.conv_fwd_fp8(y18, n, oh, ow, S.w8(blk.conv2.weight)[0], planes, 3, 1, d, d,
                                    S.st(name + ".y1"), S.w8(blk.conv2.weight)[1])
        y28 = torch.empty_like(y18)
        ops.bn_apply(c2, ev(c2, blk.bn2), blk.bn2, act=1, out8=y28, qstate=s2)
        c3, _, _ = ops.conv_fwd_fp8(y28, n, oh, ow, S.w8(blk.conv3.weight)[0], 4 * planes, 1, 1, 0, 1,
                                    S.st(name + ".y2"), S.w8(blk.conv3.weight)[1])
        r8 = torch.empty(tuple(c3.shape), dtype=torch.uint8, device=cuda)
        if index == 0:
            bnd = blk.downsample[1]
            cd, _, _ = ops.conv_fwd_fp8(x8, n, h, w, S.w8(blk.downsample[0].weight)[0], 4 * planes, 1, s, 0, 1,
                                        S.st(name + ".x"), S.w8(blk.downsample[0].weight)[1])
            ry = ops.bn_apply(c3, ev(c3, blk.bn3), blk.bn3, act=1, xr=cd, rstats=ev(cd, bnd), rbn=bnd,
                              out8=r8, qstate=so)
        else:
            ry = ops.bn_apply(c3, ev(c3, blk.bn3), blk.bn3, act=1, res=x, out8=r8, qstate=so)
    torch.cuda.synchronize()
    assert ogeo == (n, oh, ow) and y.shape == (n * oh * ow, 4 * planes)
    assert torch.isfinite(ry.float()).all() and ry.float().abs().max() > 0 and len(torch.unique(r8)) > 16
    assert torch.equal(y.view(torch.int16), ry.view(torch.int16))
    assert torch.equal(y8, r8)


# ---- 7. accuracy --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feature_errors(cuda, bf16_model, fp32_model, static_model):
    """seed -> {(modality, path): r} with r(m) = ||f_m - f_fp32|| / ||f_fp32|| over the four frames'
    features; the fp32 and bf16 banks are the existing paths, computed once per seed."""
    cache = {}

    def get(seed):
        if seed not in cache:
            X = four_frames(cuda, seed)
            truth = FeatureBank.encode(fp32_model, *X)
            out = {}
            for path, m in (("bf16", bf16_model), ("fp8", static_model)):
                b = FeatureBank.encode(m, *X)
                for mod, f, t in (("rgb", b.va, truth.va), ("depth", b.da, truth.da)):
                    out[(mod, path)] = ((f.double() - t.double()).norm() / t.double().norm()).item()
            cache[seed] = out
        return cache[seed]

    return get


@pytest.mark.parametrize("seed", [21, 23])
def test_static_fp8_features_against_fp32(feature_errors, seed):
    """r(fp8) <= 32 r(bf16) for the RGB and the depth features, calibrated on seed 20's frames.
    16 is the ratio of the unit roundoffs of e4m3 (2^-5) and bf16 (2^-9) -- both paths round the
    same operands at the same places -- and the further factor 2 is margin for that estimate and
    for seed spread.  Measured on an MI355X, r(fp8) / r(bf16) (r(bf16), r(fp8)):
        seed 21 rgb:   1.18 (5.4672e-01, 6.4543e-01)
        seed 21 depth: 2.02 (3.3821e-01, 6.8268e-01)
        seed 23 rgb:   1.24 (4.7709e-01, 5.8951e-01)
        seed 23 depth: 1.50 (3.9163e-01, 5.8902e-01)
    Caveat: the seeded-recipe network amplifies any rounding so much that the bf16 features
    already differ from fp32's by a third to a half, and the fp8 features are near the
    decorrelated level; there the ratio cannot grow, so the bound is met but hardly binds
    (DESIGN 3.6 has the per-layer growth).  The bitwise wiring test above carries the correctness."""
    e = feature_errors(seed)
    for mod in ("rgb", "depth"):
        rb, r8 = e[(mod, "bf16")], e[(mod, "fp8")]
        print("seed %d %s features vs fp32: r(bf16) %.4e, r(fp8) %.4e, ratio %.2f (bound 32)"
              % (seed, mod, rb, r8, r8 / rb))
    for mod in ("rgb", "depth"):
        rb, r8 = e[(mod, "bf16")], e[(mod, "fp8")]
        assert rb > 0 and r8 <= 32 * rb, (seed, mod, rb, r8, r8 / rb)


# ---- 8. end to end and refusals --------------------------------------------------------------------------------
def test_segment_sequence_and_indexed_head_on_a_static_model(cuda, static_model, fp32_model):
    m = static_model
    rgbs, deps = four_frames(cuda, 21)
    run = lambda mm, coatt: segment_sequence(mm, rgbs, deps, [[1, 2, 3]], targets=[0], coatt=coatt)
    x1 = run(m, "bf16")
    xm = run(m, "mxfp8")
    truth = run(fp32_model, "bf16").double().cpu()
    torch.cuda.synchronize()
    for x in (x1, xm):
        assert x.shape == (1, 1) + SIZE and x.dtype == torch.float32
        assert torch.isfinite(x).all() and x.min() >= 0 and x.max() <= 1
    for name, x in (("bf16 coatt", x1), ("mxfp8 coatt", xm)):
        x = x.double().cpu()
        print("65x81, 1 target x 3 references, static fp8 encoders, %s: mean |x1 - x1_fp32| %.4e, "
              "mask agreement %.5f" % (name, (x - truth).abs().mean().item(),
                                       ((x > 0.5) == (truth > 0.5)).double().mean().item()))
    with torch.no_grad():
        bank = FeatureBank.encode(m, rgbs, deps)
        assert bank.mx is None and m.head_a_indexed(bank, [0, 0], [1, 3]).shape == (2, 1) + SIZE


def test_refusals(cuda, bf16_model, fp32_model, static_model, calib20):
    rgbs, deps = four_frames(cuda, 21)
    with pytest.raises(ValueError):                       # fp32 model
        fp32_model.set_fp8_static(calib20)
    assert fp32_model.fp8_static is None
    with pytest.raises(ValueError):
        FI.calibrate(fp32_model, rgbs, deps)
    short = {k: dict(v) for k, v in calib20.amax.items()}
    short["encoder"].pop("aspp.cat")
    with pytest.raises(ValueError):                       # key sets differ
        bf16_model.set_fp8_static(FI.Fp8Calibration(short))
    extra = {k: dict(v) for k, v in calib20.amax.items()}
    extra["depth_encoder"]["backbone.layer9.0.x"] = 1.0
    with pytest.raises(ValueError):
        bf16_model.set_fp8_static(FI.Fp8Calibration(extra))
    assert bf16_model.fp8_static is None
    with pytest.raises(ValueError):                       # a state built for another model
        bf16_model.set_fp8_static(static_model.fp8_static)
    # the two fp8 modes exclude each other
    bf16_model.set_fp8(True)
    try:
        with pytest.raises(RuntimeError):
            bf16_model.set_fp8_static(calib20)
        with pytest.raises(RuntimeError):
            FI.calibrate(bf16_model, rgbs, deps)
        with torch.no_grad():                             # and delayed scaling stays refused by the bank head
            bank = FeatureBank.encode(static_model, rgbs, deps)
            with pytest.raises(RuntimeError):
                bf16_model.head_a_indexed(bank, [0], [1])
    finally:
        bf16_model.set_fp8(False)
    m = static_model
    with pytest.raises(RuntimeError):
        m.set_fp8(True)
    assert m.fp8 is None and m.fp8_static is not None
    with pytest.raises(RuntimeError, match="segment_sequence"):
        multi_reference_x1(m, rgbs[:1], deps[:1], rgbs[1:], deps[1:])
    with pytest.raises(RuntimeError):                     # grad enabled
        FI.encode_frames_static(m.encoder, rgbs)
    with pytest.raises(RuntimeError):                     # the pair forward, grad enabled
        m(rgbs[:1], rgbs[1:2], deps[:1], deps[1:2])
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            FI.encode_frames_static(bf16_model.encoder, rgbs)    # no static scales
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m(rgbs[:1], rgbs[1:2], deps[:1], deps[1:2])
        with pytest.raises(RuntimeError):
            FeatureBank.encode(m, rgbs, deps)
        with torch.no_grad(), pytest.raises(RuntimeError):
            FI.encode_frames_static(m.encoder, rgbs)
        with pytest.raises(RuntimeError):
            FI.calibrate(m, rgbs, deps)
    finally:
        m.eval()
    # switched off and back on with the built state
    st = m.fp8_static
    m.set_fp8_static(None)
    assert m.fp8_static is None and m.encoder._cn_fp8_static is None
    assert m.set_fp8_static(st).fp8_static is st


# ---- 9. test.py --feature-bank --dtype fp8 ------------------------------------------------------------------------
def _write_tree(root, seqs, hw=(40, 52)):
    """An SBM-RGBD tree of seeded noise frames: <root>/<category>/<sequence>/{input, depth,
    groundtruth}/ and ROI.bmp."""
    from PIL import Image
    g = np.random.default_rng(11)
    h, w = hw
    for cat, seq, nf in seqs:
        base = os.path.join(root, cat, seq)
        for d in ("input", "depth", "groundtruth"):
            os.makedirs(os.path.join(base, d), exist_ok=True)
        roi = np.zeros((h, w), np.uint8)
        roi[3:h - 4, 5:w - 2] = 255
        Image.fromarray(roi).save(os.path.join(base, "ROI.bmp"))
        for i in range(nf):
            fid = "%06d" % (10 * i + 7)
            Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
                os.path.join(base, "input", "in%s.png" % fid))
            Image.fromarray(g.integers(0, 256, (h, w), dtype=np.uint8)).save(
                os.path.join(base, "depth", "d%s.png" % fid))
            gt = (g.random((h, w)) > 0.7).astype(np.uint8) * 255
            Image.fromarray(gt).save(os.path.join(base, "groundtruth", "gt%s.png" % fid))


@pytest.fixture(scope="module")
def cli_env(tmp_path_factory):
    """A written SBM-RGBD tree (three sequences of 4-5 frames), a config for it (sample_range 2,
    65 x 81 model input) and a calibrated checkpoint."""
    import yaml
    from cosnet_amd.checkpoint import save_snapshot
    root = str(tmp_path_factory.mktemp("fp8_static_cli"))
    data = os.path.join(root, "sbm")
    _write_tree(data, seqs=(("Shadows", "s1", 4), ("OutOfRange", "s2", 5), ("OutOfRange", "s3", 4)))
    ds = {"output_WH": "52,40", "image_HW_4_model": "65, 81", "sample_range": 2, "subset": {},
          "data_path": data}
    cfg = os.path.join(root, "config.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"test": {"model": {"resnet_aspp_add": {"pretrained_params": ""}},
                                 "dataset": {"sbmrgbd": ds}}}, f)
    m = make_model(None, torch.float32)
    return root, cfg, save_snapshot(os.path.join(root, "snapshot.pth"), 1, m)


def _run_cli(env, name, extra):
    import test as test_cli
    top, cfg, ckpt = env
    root = os.path.join(top, name)
    rc = test_cli.main(["--dataset", "sbmrgbd", "--model", "raa", "--gpus", "0", "--feature-bank",
                        "--config", cfg, "--checkpoint", ckpt, "--result-root", root] + extra)
    assert rc == 0
    logs, pngs = [], {}
    for d, _, files in os.walk(root):
        logs += [os.path.join(d, f) for f in files if f.endswith("_test_log.txt")]
        for f in files:
            if f.endswith(".png"):
                with open(os.path.join(d, f), "rb") as fh:
                    pngs[os.path.relpath(os.path.join(d, f), root).split(os.sep, 4)[-1]] = fh.read()
    assert len(logs) == 1
    text = open(logs[0]).read()
    frames = re.findall(r"##== seq: (\S+) frame: (\S+) IOU: ([0-9.eE+-]+)==##", text)
    final = re.findall(r"##== final IOU: ([0-9.eE+-]+)==##", text)
    assert len(final) == 1
    return [(s, f) for s, f, _ in frames], [v for _, _, v in frames], final[0], pngs


def test_cli_dtype_fp8_calibrates_once_and_repeats(cuda, cli_env):
    """test.py --feature-bank --dtype fp8 --fp8-calibration F: the first run creates F and writes
    the seq / frame lines and PNG paths of --dtype bf16; the second loads F and repeats the first
    byte for byte (PNGs and IoU strings)."""
    F = os.path.join(cli_env[0], "calibration.json")
    a = _run_cli(cli_env, "bf16", ["--dtype", "bf16"])
    assert not os.path.exists(F)
    b = _run_cli(cli_env, "fp8_first", ["--dtype", "fp8", "--fp8-calibration", F])
    assert os.path.exists(F)
    made = open(F, "rb").read()
    calib = FI.Fp8Calibration.load(F)
    assert all(len(calib.amax[k]) > 0 for k in FI.ENCODERS)
    c = _run_cli(cli_env, "fp8_second", ["--dtype", "fp8", "--fp8-calibration", F, "--coatt", "bf16"])
    assert open(F, "rb").read() == made                       # loaded, not rewritten
    assert len(a[0]) == 13 and a[0] == b[0] == c[0]
    assert sorted(a[3]) == sorted(b[3]) == sorted(c[3]) and len(a[3]) == 13
    assert b[3] == c[3], "PNG bytes differ between the calibrating run and the run that loaded the file"
    assert b[1] == c[1] and b[2] == c[2]
    print("sbmrgbd 13 frames: final IOU bf16 bank %s, static fp8 bank %s; max per-frame |d| %.2e" % (
        a[2], b[2], max(abs(float(x) - float(y)) for x, y in zip(a[1], b[1]))))
