"""The BN fold without a GPU: the extension header's binding, the guard conditions of the exact
generators of tests/test_gpu_conv_affine.py (as tests/test_cpu_exact_inputs.py does for its own),
the command-line refusals, set_bn_fold's refusals that need no device, and the staleness rule of
FoldTables."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import REPO
import cosnet_amd as C
from cosnet_amd import _native, bn_fold, ops

import test_gpu_conv_affine as A

EXT = ["cn_bn_fold_table", "cn_conv_fwd_affine"]


# ---- T1: the binding ----------------------------------------------------------------------------------
def test_extension_header_parses_and_core_set_is_unchanged():
    with open(os.path.join(REPO, "include", "cosnet_hip_infer.h")) as fh:
        sigs = _native.signatures(fh.read())
    assert sorted(sigs) == EXT == _native.extension_symbols()
    I, L, F, S, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
    res, args, names = sigs["cn_conv_fwd_affine"]
    assert res is I and args == [I, P, L, I, I, I, I, P, I, I, I, I, I, I, P, P, L, I, I, P, P, P, L, I, P, P, S, P]
    assert names[19:] == ["scale", "shift", "res", "ldr", "act", "prelu", "ws", "ws_floats", "stream"]
    assert sigs["cn_bn_fold_table"] == (I, [P, P, P, P, I, F, P, P, P],
                                        ["run_mean", "run_var", "gamma", "beta", "C", "eps", "scale", "shift",
                                         "stream"])
    core = _native.exported_symbols()
    assert len(core) == 94 and not set(core) & set(EXT)
    # the first 19 parameters are cn_conv_fwd's without its stream: one contract for x, w, y
    with open(os.path.join(REPO, "include", "cosnet_hip.h")) as fh:
        base = _native.signatures(fh.read())["cn_conv_fwd"]
    assert (args[:19], names[:19]) == (base[1][:19], base[2][:19])


def test_library_exports_the_extension_symbols_and_hashes_the_header():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for n in EXT:
        assert hasattr(lib, n), n
    assert _native.load().cn_conv_fwd_affine.argtypes[-2] is ctypes.c_size_t
    assert _native.HASHED_SOURCES[-1] == "../../include/cosnet_hip_infer.h"
    with open(os.path.join(REPO, "cosnet_amd", "csrc", "Makefile")) as fh:
        hashed = re.search(r"^HASHED := (.*)$", fh.read(), re.M).group(1).split()
    assert hashed[-5:] == _native.HASHED_SOURCES[-5:]


# ---- T2: the generators' guard conditions ---------------------------------------------------------------
def test_affine_generators_meet_their_conditions():
    """Every comparison of test_gpu_conv_affine.py: pre-activation exact and below 2^24 with
    >= 10 % ties; after the ReLU >= 5 % ties and 40-60 % zeros (pytest -s prints the ranges)."""
    s = A.affine_scale(4000, 1)
    assert set(s.tolist()) == {0.5, 1.0, 2.0}
    pre, post, zeros = [], [], []
    for label, ap in A.all_affine_problems():
        a, b, z = A.verify_affine(ap)
        pre.append(a)
        if ap.act == 1:
            post.append(b)
            zeros.append(z)
    assert len(pre) >= 100
    print("ties before the activation %.1f-%.1f %%, after the ReLU %.1f-%.1f %%, zeros %.1f-%.1f %%" % (
        100 * min(pre), 100 * max(pre), 100 * min(post), 100 * max(post), 100 * min(zeros), 100 * max(zeros)))
    assert min(pre) >= A.MIN_TIES_PRE and min(post) >= A.MIN_TIES_RELU
    assert A.ZEROS[0] <= min(zeros) and max(zeros) <= A.ZEROS[1]


def test_act_reference():
    t = torch.tensor([-8.0, -0.5, 0.0, 3.0], dtype=torch.float64)
    assert A.act_of(t, 0).tolist() == [-8.0, -0.5, 0.0, 3.0]
    assert A.act_of(t, 1).tolist() == [0.0, 0.0, 0.0, 3.0]
    assert A.act_of(t, 2).tolist() == [-2.0, -0.125, 0.0, 3.0]


# ---- T3c: refusals and staleness ---------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--fold-bn"], ["--feature-bank", "--fold-bn", "--dtype", "fp8"]])
def test_cli_refuses_fold_bn_without_bank_or_with_fp8(argv, capsys):
    import test as test_cli
    with pytest.raises(SystemExit) as e:
        test_cli.get_arguments(["--dataset", "synthetic"] + argv)
    assert e.value.code == 2 and "--fold-bn" in capsys.readouterr().err
    assert test_cli.get_arguments(["--dataset", "synthetic", "--feature-bank", "--fold-bn"]).fold_bn


@pytest.fixture(scope="module")
def model_cpu():
    return C.build_model(torch.bfloat16).eval()


def test_set_bn_fold_refusals_without_a_device(model_cpu):
    m = model_cpu
    assert m.bn_fold is None and m.set_bn_fold(False) is m
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.set_bn_fold()
    finally:
        m.eval()
    m.fp8 = object()          # as set_fp8(True) leaves it
    try:
        with pytest.raises(RuntimeError, match="set_fp8"):
            m.set_bn_fold()
    finally:
        m.fp8 = None
    m.fp8_static = object()
    try:
        with pytest.raises(RuntimeError, match="set_fp8_static"):
            m.set_bn_fold()
    finally:
        m.fp8_static = None
    with pytest.raises(RuntimeError, match="GPU"):
        m.set_bn_fold()       # a CPU model: no device to build the tables on
    m.bn_fold = object()      # as set_bn_fold() leaves it
    try:
        x, d = torch.zeros(1, 3, 33, 33), torch.zeros(1, 1, 33, 33)
        with pytest.raises(RuntimeError, match="segment_sequence"):
            m(x, x, d, d)
        from cosnet_amd.inference import multi_reference_x1
        with pytest.raises(RuntimeError, match="segment_sequence"):
            multi_reference_x1(m, x, d, x, d)
        with pytest.raises(RuntimeError, match="set_bn_fold"):
            m.set_fp8(True)
        with pytest.raises(RuntimeError, match="set_bn_fold"):
            m.set_fp8_static(object())
    finally:
        m.bn_fold = None


def test_fold_tables_follow_the_version_counters(monkeypatch):
    """A table is rebuilt when one of the BN's four tensors changed (in place, or replaced), and
    only then.  The launch is replaced by the same arithmetic in torch: no device needed."""
    calls = []

    def table(bn, out=None):
        calls.append(bn)
        is_ = 1.0 / torch.sqrt(bn.running_var + bn.eps)
        sc = (bn.weight if bn.affine else torch.ones_like(is_)) * is_
        out[0].copy_(sc)
        out[1].copy_((bn.bias if bn.affine else torch.zeros_like(is_)) - bn.running_mean * sc)
        return out[0], out[1]

    monkeypatch.setattr(ops, "bn_fold_table", table)
    root = nn.Sequential(nn.Conv2d(4, 8, 1), nn.BatchNorm2d(8), nn.Sequential(nn.BatchNorm2d(8, affine=False))).eval()
    with torch.no_grad():
        T = bn_fold.FoldTables(root)
        assert len(T) == 2 and sorted(T.paths.values()) == ["1", "2.0"] and len(calls) == 2
        a, b = root[1], root[2][0]
        sc, sf = T.get(a)
        T.get(a), T.get(b)
        assert len(calls) == 2 and not T.stale(a)                  # nothing changed: no launch
        assert torch.allclose(sc, torch.full((8,), 1.0 / (1.0 + 1e-5) ** 0.5), rtol=1e-6, atol=0)
        for i, t in enumerate((a.running_mean, a.running_var, a.weight, a.bias)):
            t.add_(0.5)                                            # in place: the version counter
            assert T.stale(a) and not T.stale(b)
            sc2, sf2 = T.get(a)
            assert len(calls) == 3 + i and sc2.data_ptr() == sc.data_ptr()   # rewritten in place
        assert torch.allclose(sf2, 0.5 - 0.5 * sc2)
        root.load_state_dict({k: v.clone() for k, v in root.state_dict().items()})
        assert T.stale(a) and T.stale(b)
        T.get(b)
        assert calls[-1] is b
    with pytest.raises(ValueError, match="running statistics"):
        bn_fold.FoldTables(nn.Sequential(nn.BatchNorm2d(4, track_running_stats=False)))
