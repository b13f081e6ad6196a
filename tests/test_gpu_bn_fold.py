"""Eval-mode BatchNorm folded into the conv GEMMs (cosnet_amd/bn_fold.py, model.set_bn_fold,
test.py --feature-bank --fold-bn).

* fp32, bitwise: the folded walk of both encoders is encoder.features_nhwc (the wiring test:
  every conv, stride, dilation, residual, downsample, concat slice and the PReLU);
* bf16 blocks against fp64 of the folded math on the same bf16 operands;
* the model: segment_sequence with the fold in fp32 on the oracle's bound, in bf16 against the
  default bf16 bank's error;
* behaviour: independence of the frames encoded in between, load_state_dict, switching off, the CLI.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from cosnet_amd import bn_fold as BF
from cosnet_amd import encoder_fn as E
from cosnet_amd import ops
from cosnet_amd.inference import FeatureBank, segment_sequence
from cosnet_amd.init_recipe import synthetic_inputs

import test_gpu_feature_bank as FB
from test_gpu_feature_bank import cli_env, _run_cli, make_model  # noqa: F401  (cli_env: a fixture)

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
SIZE = (65, 81)
TOL_BF16 = 1.2e-2     # DESIGN §1's kernel bound, relative to the output scale


@pytest.fixture(scope="module")
def fp32_model(cuda):
    return make_model(cuda, torch.float32, "bn_calibration.npz")


@pytest.fixture(scope="module")
def bf16_model(cuda):
    return make_model(cuda, bf, "bn_calibration.npz")


@pytest.fixture
def folded(request):
    """set_bn_fold() on a module-scoped model for one test, off again afterwards."""
    def on(m):
        m.set_bn_fold()
        request.addfinalizer(lambda: m.set_bn_fold(False))
        return m
    return on


def frames(cuda, n, seed):
    ra, rb, da, db, _, _ = synthetic_inputs(n, SIZE[0], SIZE[1], seed=seed, correlated=False)
    return torch.cat([ra[:1], rb]).to(cuda), torch.cat([da[:1], db]).to(cuda)


# ---- T4: the wiring, fp32, bitwise ------------------------------------------------------------------
def test_folded_walk_fp32_is_bitwise_features_nhwc(cuda, fp32_model, folded):
    """3 frames at 65 x 81, both encoders (their ASPP dilations differ): cn_bn_fold_table feeds
    encode_frames_folded and the output is torch.equal to the unfolded walk's.  Every class runs
    the generic folded epilogue on the tile the unfolded conv takes (fold_route folds all)."""
    m = folded(fp32_model)
    rgbs, deps = frames(cuda, 2, 41)
    assert rgbs.shape[0] == 3
    with torch.no_grad():
        m._set_dtype()
        for enc, x in ((m.encoder, rgbs), (m.depth_encoder, deps)):
            ref, geo = enc.features_nhwc(x)
            got, ggeo = BF.encode_frames_folded(enc, x)
            torch.cuda.synchronize()
            assert ggeo == geo == (3, 9, 11) and got.dtype == torch.float32 and got.shape == ref.shape
            assert torch.isfinite(ref).all() and ref.abs().max() > 0
            assert torch.equal(got, ref), (got - ref).abs().max().item()
    n_bn = sum(1 for mod in m.encoder.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    assert len(m.bn_fold.encoders["encoder"]) == n_bn and len(m.bn_fold.head) == 2


# ---- T5: bf16 blocks against fp64 of the folded math -----------------------------------------------
def _q(t):
    """A bf16 storage point of the folded path."""
    return t.to(bf).double()


def _w64(conv):
    return conv.weight.detach().to(bf).double().cpu()


def _fold64(T, bn):
    sc, sf = T.get(bn)
    return sc.double().cpu().view(1, -1, 1, 1), sf.double().cpu().view(1, -1, 1, 1)


def _cbn64(T, x, conv, bn, stride=1, pad=0, dil=1, res=None, act=1, prelu=None):
    """fp64 of one folded launch on bf16 operands (NCHW, CPU): act(conv * scale + shift + res),
    rounded to bf16 where the launch stores."""
    bias = None if conv.bias is None else conv.bias.detach().double().cpu()
    sc, sf = _fold64(T, bn)
    t = Fn.conv2d(x, _w64(conv), bias, stride, pad, dil) * sc + sf
    if res is not None:
        t = t + res
    if act == 1:
        t = torch.relu(t)
    elif act == 2:
        t = torch.where(t > 0, t, prelu.detach().double().cpu() * t)
    return _q(t)


def _nchw(rows, n, h, w):
    return rows.double().cpu().view(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def _rows(x4):
    return x4.permute(0, 2, 3, 1).reshape(-1, x4.shape[1])


def _block_input(cuda, n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn((n * h * w, c), generator=g)).to(bf).to(cuda)


def _report(tag, got, unfolded, ref):
    s = ref.abs().max().item()
    e_f = (got.double().cpu() - ref).abs().max().item() / s
    e_u = (unfolded.double().cpu() - ref).abs().max().item() / s
    print("%s bf16 vs fp64 of the folded math: folded %.3e, unfolded %.3e of the output scale (bound %.1e)" % (
        tag, e_f, e_u, TOL_BF16))
    assert torch.isfinite(got.float()).all() and s > 0
    assert e_f <= TOL_BF16, (tag, e_f)


def _bottleneck64(T, blk, x4):
    s, d = blk.stride, blk.dilation
    y1 = _cbn64(T, x4, blk.conv1, blk.bn1, stride=s)
    y2 = _cbn64(T, y1, blk.conv2, blk.bn2, pad=d, dil=d)
    res = x4 if blk.downsample is None else _cbn64(T, x4, blk.downsample[0], blk.downsample[1], stride=s, act=0)
    return _cbn64(T, y2, blk.conv3, blk.bn3, res=res)


@pytest.mark.parametrize("which", ["layer3 identity", "layer2 stride-2 downsample"])
def test_bottleneck_bf16_matches_fp64_of_the_folded_math(cuda, bf16_model, folded, which):
    m = folded(bf16_model)
    T = m.bn_fold.encoders["encoder"]
    if which.startswith("layer3"):
        blk, (n, h, w) = m.encoder.backbone.layer3[3], (2, 9, 11)
        assert blk.downsample is None
    else:
        blk, (n, h, w) = m.encoder.backbone.layer2[0], (2, 17, 21)
        assert blk.downsample is not None and blk.stride == 2
    x = _block_input(cuda, n, h, w, blk.conv1.weight.shape[1], 5)
    with torch.no_grad():
        m._set_dtype()
        got, geo = BF.bottleneck_folded(blk, x, (n, h, w), T)
        unf, ugeo = E.bottleneck_fwd(blk, x, (n, h, w), 1, None)
    torch.cuda.synchronize()
    assert geo == ugeo == (2, 9, 11)
    _report(which, got, unf, _rows(_bottleneck64(T, blk, _nchw(x, n, h, w))))


def test_aspp_bf16_matches_fp64_of_the_folded_math(cuda, bf16_model, folded):
    m = folded(bf16_model)
    T, mod = m.bn_fold.encoders["encoder"], m.encoder.aspp
    n, h, w = 2, 9, 11
    x = _block_input(cuda, n, h, w, 2048, 6)
    with torch.no_grad():
        m._set_dtype()
        got = BF.aspp_folded(mod, x, (n, h, w), T)
        unf = E.aspp_fwd(mod, x, (n, h, w), 1, None)
    torch.cuda.synchronize()
    x4 = _nchw(x, n, h, w)
    pool = _q(x4.mean(dim=(2, 3), keepdim=True))
    parts = [_cbn64(T, pool, mod.conv, mod.bn_x).expand(n, 512, h, w)]
    for cm, bnm, k, dd in E.aspp_branches(mod):
        parts.append(_cbn64(T, x4, cm, bnm, pad=dd, dil=max(dd, 1)))
    ref = _cbn64(T, torch.cat(parts, 1), mod.bottleneck, mod.bn, pad=1, act=2, prelu=mod.prelu.weight)
    _report("ASPP", got, unf, _rows(ref))


# ---- T6: the model, fp32, on the oracle's bound ----------------------------------------------------
def test_segment_sequence_fp32_folded_matches_oracle_loop_mean(cuda, fp32_model, folded):
    """The inputs, refs, chunks and bound of
    test_gpu_feature_bank.py::test_segment_sequence_fp32_matches_oracle_loop_mean with
    set_bn_fold(): 8 x the oracle's own fp32-vs-fp64 floor + 1e-5, no mask flips outside the band."""
    from oracle.model_ref import RefModel
    refs = [[1, 2], [0, 0], [3, 2], [2, 1]]
    ra, rb, da, db, _, _ = synthetic_inputs(2, 65, 81, seed=33, correlated=False)
    rgbs, deps = torch.cat([ra, rb]), torch.cat([da, db])
    m = folded(fp32_model)
    sd = FB._SD["bn_calibration.npz"]
    got = segment_sequence(m, rgbs.to(cuda), deps.to(cuda), refs, encode_chunk=3, pair_chunk=4)
    torch.cuda.synchronize()
    assert got.shape == (4, 1, 65, 81) and got.dtype == torch.float32
    ta = [t for t, r in enumerate(refs) for _ in r]
    tb = [j for r in refs for j in r]
    truth = {}
    for dt in (torch.float64, torch.float32):
        ref = RefModel(sd, dtype=dt, requires_grad=False)
        ref.training = False
        with torch.no_grad():
            x1, _, _ = ref.forward(rgbs[ta].to(dt), rgbs[tb].to(dt), deps[ta].to(dt), deps[tb].to(dt))
        x1 = x1.reshape(4, 2, 65 * 81)
        acc = x1[:, 0].clone()
        acc += x1[:, 1]
        truth[dt] = (acc / 2).double().numpy()
    r64 = truth[torch.float64]
    floor = float(np.abs(truth[torch.float32] - r64).max())
    tol = 8 * floor + 1e-5
    g = got.double().cpu().numpy().reshape(4, -1)
    for t in range(4):
        err = float(np.abs(g[t] - r64[t]).max())
        print("folded segment_sequence fp32 target %d: max err %.3e (tol %.3e, oracle floor %.3e)" % (t, err, tol, floor))
        assert err <= tol, (t, err, tol, floor)
        amb = np.abs(r64[t] - 0.5) <= tol
        flips = ((g[t] > 0.5) != (r64[t] > 0.5)) & ~amb
        assert not flips.any(), (t, int(flips.sum()))


# ---- T7: the model, bf16, against the default bank's error ------------------------------------------
def test_folded_bank_bf16_error_against_fp32(cuda, bf16_model, fp32_model):
    """Truth: the fp32 default path.  Mean |x1 - x1_fp32| of the folded bf16 bank may exceed the
    default bf16 bank's by at most 1.5 x (the margin tests/test_gpu_feature_bank_mxfp8.py gives the
    same quantity), on seeds 21 / 22 / 23 at 65 x 81, one target with three references.  Measured on
    an MI355X, folded / default (default, folded; folded mask agreement 1.0 in every case):
        seed 21: 1.1092 (3.0432e-04, 3.3754e-04)
        seed 22: 1.4988 (5.3933e-06, 8.0832e-06)
        seed 23: 0.3487 (5.4401e-04, 1.8970e-04)
    Both paths are deterministic, so seed 22's ratio does not move from run to run; its errors are
    two orders below the other seeds' (a bank whose x1 barely depends on the features)."""
    ratios = []
    for seed in (21, 22, 23):
        rgbs, deps = frames(cuda, 3, seed)
        run = lambda m: segment_sequence(m, rgbs, deps, [[1, 2, 3]], targets=[0]).double().cpu()
        truth, default = run(fp32_model), run(bf16_model)
        bf16_model.set_bn_fold()
        try:
            fold = run(bf16_model)
        finally:
            bf16_model.set_bn_fold(False)
        e_d, e_f = (default - truth).abs().mean().item(), (fold - truth).abs().mean().item()
        agree = ((fold > 0.5) == (truth > 0.5)).double().mean().item()
        print("seed %d: default bf16 bank mean |d| %.4e, folded %.4e, ratio %.4f, folded mask agreement %.5f" % (
            seed, e_d, e_f, e_f / e_d, agree))
        assert torch.isfinite(fold).all() and fold.min() >= 0 and fold.max() <= 1
        ratios.append((e_f, e_d))
    for e_f, e_d in ratios:
        assert e_f <= 1.5 * e_d, ratios


# ---- T8: behaviour ----------------------------------------------------------------------------------
def test_fold_is_stateless_follows_load_state_dict_and_switches_off(cuda, monkeypatch):
    """fp32, where the folded walk is bitwise the default one: any stale table or leftover state
    shows as a differing bit."""
    m = make_model(cuda, torch.float32, "bn_calibration.npz")       # its own model: the state changes
    rgbs, deps = frames(cuda, 3, 9)
    calls = []
    real = ops.conv_fwd_affine
    monkeypatch.setattr(ops, "conv_fwd_affine", lambda *a, **k: calls.append(1) or real(*a, **k))
    enc = lambda: FeatureBank.encode(m, rgbs[:2], deps[:2], encode_chunk=2)
    same = lambda x, y: all(torch.equal(getattr(x, k), getattr(y, k)) for k in ("va", "da", "vat", "dat"))
    with torch.no_grad():
        base = enc()
        assert not calls
        m.set_bn_fold()
        a = enc()
        per_pass = len(calls)
        # one launch per conv + BN pair: every BatchNorm2d of the two encoders, once
        assert per_pass == sum(len(t) for t in m.bn_fold.encoders.values()) == 169
        FeatureBank.encode(m, rgbs[2:], deps[2:])                   # other frames in between
        b = enc()
        assert same(a, b) and same(a, base)
        # other running statistics: the tables are rebuilt and the features follow
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd2 = {k: (v * 1.5 if k.endswith("running_var") else v) for k, v in sd.items()}
        m.load_state_dict(sd2)
        c = enc()
        assert not torch.equal(c.va, a.va)
        m.set_bn_fold(False)
        assert m.bn_fold is None
        n = len(calls)
        c_default = enc()
        assert len(calls) == n                                      # switched off: the default path runs
        assert same(c, c_default)
        m.load_state_dict(sd)
        assert same(enc(), base)
    with pytest.raises(RuntimeError, match="fold tables"):
        with torch.no_grad():
            BF.encode_frames_folded(m.encoder, rgbs)


def test_set_bn_fold_refusals_on_the_device(cuda, bf16_model, folded):
    m = folded(bf16_model)
    rgbs, deps = frames(cuda, 1, 3)
    with pytest.raises(RuntimeError, match="segment_sequence"):
        m(rgbs[:1], rgbs[1:], deps[:1], deps[1:])
    with pytest.raises(RuntimeError, match="set_bn_fold"):
        m.set_fp8(True)
    with pytest.raises(RuntimeError, match="eval mode"):
        BF.encode_frames_folded(m.encoder, rgbs)                    # grad mode
    m.set_bn_fold(False)
    m.set_fp8(True)
    try:
        with pytest.raises(RuntimeError, match="set_fp8"):
            m.set_bn_fold()
    finally:
        m.set_fp8(False)


def test_cli_fold_bn_is_repeatable_and_keeps_the_iou(cuda, cli_env):
    """test.py --feature-bank --fold-bn twice: byte-identical PNGs; final IoU within 0.002 of
    --feature-bank (fp32, where the folded encoders are bitwise the default ones)."""
    base = _run_cli(cli_env, "sbmrgbd", "bank_default", ["--feature-bank"])
    runs = [_run_cli(cli_env, "sbmrgbd", "bank_fold%d" % i, ["--feature-bank", "--fold-bn"]) for i in (1, 2)]
    assert runs[0][0] == runs[1][0] == base[0] and runs[0][3] == runs[1][3] == base[3]
    top = cli_env[0]
    for rel in runs[0][3]:
        files = []
        for i in (1, 2):
            hits = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(top, "sbmrgbd_bank_fold%d" % i))
                    for f in fs if os.path.join(d, f).endswith(rel)]
            assert len(hits) == 1, (rel, hits)
            files.append(open(hits[0], "rb").read())
        assert files[0] == files[1], rel
    print("final IOU --feature-bank %.6f, --fold-bn %.6f" % (base[2], runs[0][2]))
    assert abs(runs[0][2] - base[2]) <= 0.002, (runs[0][2], base[2])
