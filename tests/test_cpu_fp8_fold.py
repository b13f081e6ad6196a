"""The static-fp8 BN fold without a GPU: the header binding of cn_conv_fwd_fp8_affine, the
command-line rules of test.py --fp8-fold-bn, and the guard conditions of the exact inputs of
tests/test_gpu_conv_fp8_affine.py.

The exact problem is tests/test_gpu_exact_gemm.py's fp8 forward problem (decoded integer operands,
FP8_SX = 0.5, FP8_SW = 0.25, its bias) behind tests/test_gpu_conv_affine.py's affine:
scale = affine_scale(cout, 7001), shift = offset_bias(cout, 7002), res = old_c(shape, 7003), acts
0 / 1 / 2, output inverse scales 1/2 and 1/8.  Every combination of (act, res / none, bias / none)
must be exact (partial sums below 2^24, t * qinv exact in fp32) -- that is what makes the GPU
comparison bitwise.  The shares that keep it from being vacuous -- bf16 ties, e4m3 saturation,
inexact e4m3 values, exact e4m3 ties -- are conditions of the full problem (residual and bias
present: without the two offsets nothing reaches +-896, so nothing saturates at qinv = 1/2); the
reduced combinations are compared all the same.
"""
import ctypes
import os

import pytest
import torch

from conftest import REPO
from cosnet_amd import _native

import test_gpu_exact_gemm as E
import test_gpu_conv_affine as A

E4M3 = torch.float8_e4m3fn
QINVS = (0.5, 0.125)
SEED_SCALE, SEED_SHIFT, SEED_RES = 7001, 7002, 7003


# ---- the exact problem (shared with tests/test_gpu_conv_fp8_affine.py) ------------------------------
def fold_problem(case, act, with_res, with_bias):
    """(pr, scale, shift, res, t, bound): t [n, cout, oh, ow] fp64 is the exact value of
    act(fma(acc * sx * sw + bias, scale, shift) + res); bound the largest partial sum."""
    n, cin, h, w, cout, k, s, p, d = case
    pr = E.fp8_fwd_problem(case)
    y = pr.outs["fwd"].ref
    acc = y if with_bias else y - pr.bias.view(1, -1, 1, 1)
    scale, shift = A.affine_scale(cout, SEED_SCALE), E.offset_bias(cout, SEED_SHIFT)
    res = E.old_c(acc.shape, SEED_RES) if with_res else None
    pre = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if res is not None:
        pre = pre + res
    bound = (2 * E.bound_of(k * k * cin, pr.xb, pr.wb, pr.bias if with_bias else None)
             + E.amax(shift) + E.amax(res))
    return pr, scale, shift, res, A.act_of(pre, act), bound


def e4m3_of(t, qinv):
    """The bytes the contract names: clamp(t * qinv, +-448) as fp32, converted by torch (RNE)."""
    return (t * qinv).clamp(-448.0, 448.0).float().to(E4M3)


def e4m3_tie(u):
    """u (fp64, |u| <= 448) lies exactly halfway between two e4m3 neighbours."""
    a = u.abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -20))).clamp(-6, 8)
    r = a / torch.pow(2.0, e - 3)          # in units of the binade's spacing (2^-9 for subnormals)
    return (r - torch.floor(r)) == 0.5


def shares(t, qinv):
    """(saturating, in range and inexact, exact ties) shares of t * qinv in e4m3."""
    u = t * qinv
    inr = u.abs() <= 448.0
    q = e4m3_of(t, qinv).double()
    inexact = inr & (q != u)
    return ((~inr).double().mean().item(), inexact.double().mean().item(),
            (inr & e4m3_tie(u)).double().mean().item())


def test_e4m3_tie_predicate():
    u = torch.tensor([17.0, 18.0, 19.0, 0.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, 232.0, 240.0, 0.3], dtype=torch.float64)
    # spacing 2 in [16, 32): 17 and 19 are ties; 2^-10 and 3 * 2^-10 are subnormal ties; 232 is
    # the tie between 224 and 240
    assert e4m3_tie(u).tolist() == [True, False, True, False, True, True, False, True, False, False]
    # RNE: ties go to the even mantissa
    assert torch.tensor([17.0, 19.0, 232.0]).to(E4M3).float().tolist() == [16.0, 20.0, 224.0]


# ---- the binding ----------------------------------------------------------------------------------------
def test_fp8_affine_prototype_is_bound_from_its_header():
    with open(os.path.join(REPO, "include", "cosnet_hip_infer_fp8.h")) as fh:
        sigs = _native.signatures(fh.read())
    assert sorted(sigs) == ["cn_conv_fwd_fp8_affine"] == _native.fp8_extension_symbols()
    I, L, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    res, args, names = sigs["cn_conv_fwd_fp8_affine"]
    assert res is I
    assert args == [P, L, I, I, I, I, P, I, I, I, I, I, I, P, P, P, P, P, P, L, I, P, P, L, P, L, P, I, I, P]
    assert names == ["x8", "ldx", "N", "H", "W", "Cin", "w8", "Cout", "KH", "KW", "stride", "pad", "dil",
                     "bias", "x_state", "w_state", "scale", "shift", "res", "ldr", "act", "prelu",
                     "y", "ldy", "y8", "ldy8", "out_state", "OH", "OW", "st"]
    # the operands are cn_conv_fwd_fp8's, in its order
    with open(os.path.join(REPO, "include", "cosnet_hip.h")) as fh:
        base = _native.signatures(fh.read())["cn_conv_fwd_fp8"]
    assert (args[:14], names[:14]) == (base[1][:14], base[2][:14])
    # the core and the bf16 extension sets are untouched
    assert "cn_conv_fwd_fp8_affine" not in _native.exported_symbols() + _native.extension_symbols()
    assert _native._signature("cn_conv_fwd_fp8_affine") == sigs["cn_conv_fwd_fp8_affine"]
    assert "../../include/cosnet_hip_infer_fp8.h" in _native.HASHED_SOURCES
    with open(os.path.join(REPO, "cosnet_amd", "csrc", "Makefile")) as fh:
        import re
        hashed = re.search(r"^HASHED := (.*)$", fh.read(), re.M).group(1).split()
    assert hashed[1:] == _native.HASHED_SOURCES[len(_native.HASHED_SOURCES) - len(hashed) + 1:]


# ---- the command line -------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--fp8-fold-bn"], ["--fp8-fold-bn", "--feature-bank"],
                                  ["--fp8-fold-bn", "--dtype", "fp8"],
                                  ["--fold-bn", "--feature-bank", "--dtype", "fp8"]])
def test_cli_refusals(argv, capsys):
    import test as test_cli
    with pytest.raises(SystemExit) as e:
        test_cli.get_arguments(["--dataset", "synthetic"] + argv)
    assert e.value.code == 2
    if argv[0] == "--fp8-fold-bn" and "--dtype" not in argv:
        assert "--fp8-fold-bn" in capsys.readouterr().err


def test_cli_parses_fp8_fold_bn():
    import test as test_cli
    a = test_cli.get_arguments(["--dataset", "synthetic", "--fp8-fold-bn", "--feature-bank", "--dtype", "fp8"])
    assert a.fp8_fold_bn and a.feature_bank and a.dtype == "fp8" and not a.fold_bn
    a = test_cli.get_arguments(["--dataset", "synthetic", "--feature-bank", "--dtype", "fp8"])
    assert not a.fp8_fold_bn


# ---- the guards ---------------------------------------------------------------------------------------------
def test_exact_inputs_meet_their_guards():
    sat2, inex2, inex8, ties8, bties = [], [], [], [], []
    for case in E.FP8_FWD_CASES:
        for act in A.ACTS:
            for with_res in (False, True):
                for with_bias in (False, True):
                    pr, scale, shift, res, t, bound = fold_problem(case, act, with_res, with_bias)
                    assert bound < 2 ** 24, bound                       # every partial sum
                    assert torch.equal(t.to(torch.float32).double(), t)
                    for qinv in QINVS:                                   # t * qinv is exact in fp32
                        u = t * qinv
                        assert torch.equal(u.to(torch.float32).double(), u)
                    if not (with_res and with_bias):
                        continue
                    label = (case, act)
                    b = E.tie_share(t)
                    assert b >= E.MIN_TIES, (label, b)
                    s2, i2, _ = shares(t, 0.5)
                    assert s2 >= 0.20 and i2 >= 0.10, (label, s2, i2)
                    s8, i8, t8 = shares(t, 0.125)
                    assert s8 == 0.0 and i8 >= 0.40 and t8 >= 0.005, (label, s8, i8, t8)
                    sat2.append(s2), inex2.append(i2), inex8.append(i8), ties8.append(t8), bties.append(b)
    rng = lambda v: "%.1f-%.1f %%" % (100 * min(v), 100 * max(v))
    print("bf16 ties %s; qinv 1/2: saturating %s, inexact in range %s; qinv 1/8: inexact %s, exact ties %s"
          % (rng(bties), rng(sat2), rng(inex2), rng(inex8), rng(ties8)))
    assert len(sat2) == 3 * len(E.FP8_FWD_CASES)
