"""Static-scale fp8 inference, the parts that need no GPU: test.py's --dtype fp8 arguments and the
Fp8Calibration record (JSON round trip bit for bit, format version, key sets against a model)."""
import json
import struct

import numpy as np
import pytest
import torch

import cosnet_amd as C
from cosnet_amd import fp8_infer as FI
import test as test_cli


# ---- test.py arguments ---------------------------------------------------------------------------
def test_dtype_fp8_options_and_defaults():
    a = test_cli.get_arguments(["--feature-bank", "--dtype", "fp8"])
    assert (a.dtype, a.feature_bank, a.coatt) == ("fp8", True, "bf16")
    assert a.fp8_calibration is None and a.fp8_calibration_frames == 16
    a = test_cli.get_arguments(["--feature-bank", "--dtype", "fp8", "--coatt", "mxfp8",
                                "--fp8-calibration", "c.json", "--fp8-calibration-frames", "4"])
    assert (a.dtype, a.coatt, a.fp8_calibration, a.fp8_calibration_frames) == ("fp8", "mxfp8", "c.json", 4)
    assert test_cli.get_arguments([]).dtype == "bf16"


@pytest.mark.parametrize("argv,message", [
    (["--dtype", "fp8"], "--dtype fp8 needs --feature-bank"),
    (["--dtype", "fp8", "--fp8-calibration", "c.json"], "--dtype fp8 needs --feature-bank"),
    (["--feature-bank", "--dtype", "bf16", "--fp8-calibration", "c.json"], "--fp8-calibration needs --dtype fp8"),
    (["--feature-bank", "--dtype", "fp8", "--fp8-calibration-frames", "0"],
     "--fp8-calibration-frames must be at least 1"),
    (["--feature-bank", "--dtype", "fp4"], "argument --dtype: invalid choice: 'fp4'"),
])
def test_dtype_fp8_refusals(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        test_cli.get_arguments(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


# ---- Fp8Calibration --------------------------------------------------------------------------------
def f32_bits(v):
    return struct.pack("<f", v)


@pytest.fixture(scope="module")
def model():
    return C.build_model(torch.bfloat16)


def seeded_calibration(model, seed=1):
    """fp32 values of every magnitude (subnormal and huge included) under the model's names."""
    g = np.random.default_rng(seed)
    amax = {}
    for k in FI.ENCODERS:
        names = FI.state_names(getattr(model, k))
        v = np.exp(g.uniform(-30, 30, len(names))).astype(np.float32)
        v[0], v[1], v[2] = np.float32(1e-42), np.float32(3.0e38), np.float32(0.0)
        amax[k] = {n: float(x) for n, x in zip(names, v)}
    return FI.Fp8Calibration(amax, margin=1.25)


def test_state_names_are_module_paths(model):
    names = FI.state_names(model.encoder)
    paths = dict(model.encoder.named_modules())
    assert len(names) == len(set(names))
    assert names[:3] == ["backbone.layer1.0.x", "backbone.layer1.0.y1", "backbone.layer1.0.y2"]
    assert names[-2:] == ["aspp.x", "aspp.cat"]
    assert all(n.rsplit(".", 1)[0] in paths for n in names)
    assert FI.state_names(model.depth_encoder)[-1] == "aspp.cat"
    ws = FI.fp8_conv_weights(model.encoder)
    assert all(w.shape[1] % 16 == 0 for w in ws)          # the eligibility rule of fp8_ok
    n_blocks = len(names) // 3
    assert len(ws) == 3 * n_blocks + 4 + 5                # + 4 downsample convs, 4 branches, bottleneck


def test_json_round_trip_is_bit_exact(model, tmp_path):
    c = seeded_calibration(model)
    path = str(tmp_path / "calib.json")
    c.save(path)
    back = FI.Fp8Calibration.load(path)
    assert back == c and back.margin == 1.25 and back.version == FI.FORMAT_VERSION
    for k in FI.ENCODERS:
        assert set(back.amax[k]) == set(c.amax[k])
        for n, v in c.amax[k].items():
            assert f32_bits(back.amax[k][n]) == f32_bits(v), (k, n)
    c.check_model(model)
    back.check_model(model)
    d = json.load(open(path))
    assert set(d) == {"format", "version", "margin", "amax"} and set(d["amax"]) == set(FI.ENCODERS)


def test_version_and_format_are_checked(model, tmp_path):
    c = seeded_calibration(model)
    path = str(tmp_path / "calib.json")
    c.save(path)
    d = json.load(open(path))
    for change in ({"version": FI.FORMAT_VERSION + 1}, {"version": None}, {"format": "something else"},
                   {"amax": {"encoder": d["amax"]["encoder"]}}, {"margin": 0.0}):
        bad = str(tmp_path / "bad.json")
        with open(bad, "w") as fh:
            json.dump(dict(d, **change), fh)
        with pytest.raises(ValueError):
            FI.Fp8Calibration.load(bad)
    with pytest.raises(ValueError):
        FI.Fp8Calibration({"encoder": {"aspp.x": float("nan")}, "depth_encoder": {}})
    with pytest.raises(ValueError):
        FI.Fp8Calibration({"encoder": {"aspp.x": -1.0}, "depth_encoder": {}})


def test_key_mismatch_is_an_error(model):
    c = seeded_calibration(model)
    missing = {k: dict(v) for k, v in c.amax.items()}
    missing["encoder"].pop("aspp.cat")
    with pytest.raises(ValueError, match="encoder"):
        FI.Fp8Calibration(missing).check_model(model)
    unknown = {k: dict(v) for k, v in c.amax.items()}
    unknown["depth_encoder"]["backbone.layer9.0.x"] = 1.0
    with pytest.raises(ValueError, match="depth_encoder"):
        FI.Fp8Calibration(unknown).check_model(model)
    # before anything touches the device: the model's own checks come first
    with pytest.raises(ValueError):
        C.build_model(torch.float32).set_fp8_static(c)
    with pytest.raises(ValueError):
        model.set_fp8_static(FI.Fp8Calibration(missing))
