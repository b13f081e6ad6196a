"""The split bank head without a GPU: the new header's binding, the hashed-source lists, the
command-line refusal, the algebra of the weight split, the guard conditions of the exact generators
of tests/test_gpu_conv_affine_add.py, and the refusals that need no device."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
import cosnet_amd as C
from cosnet_amd import _native, ops

import test_gpu_conv_affine as A
import test_gpu_conv_affine_add as D

HEAD = ["cn_conv_fwd_affine_add", "cn_conv_fwd_partial"]


def _header(name):
    with open(os.path.join(REPO, "include", name)) as fh:
        return _native.signatures(fh.read())


# ---- the binding ------------------------------------------------------------------------------------
def test_head_header_parses_and_the_other_sets_are_unchanged():
    sigs = _header("cosnet_hip_infer_head.h")
    assert sorted(sigs) == HEAD == _native.head_extension_symbols()
    I, L, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    base = _header("cosnet_hip.h")["cn_conv_fwd"]
    res, args, names = sigs["cn_conv_fwd_affine_add"]
    # the first 19 parameters are cn_conv_fwd's without its stream: one contract for x, w, y
    assert res is I and (args[:19], names[:19]) == (base[1][:19], base[2][:19])
    assert names[19:] == ["scale", "shift", "add", "lda", "add_map", "add_rows", "act", "prelu", "stream"]
    assert args[19:] == [P, P, P, L, P, I, I, P, P]
    assert sigs["cn_conv_fwd_partial"] == base          # cn_conv_fwd's operands, stream included
    core = _native.exported_symbols()
    assert len(core) == 94 and not set(core) & set(HEAD)
    assert _native.extension_symbols() == ["cn_bn_fold_table", "cn_conv_fwd_affine"]
    assert _native.fp8_extension_symbols() == ["cn_conv_fwd_fp8_affine"]
    for n in HEAD:
        assert _native._signature(n) is sigs[n] or _native._signature(n) == sigs[n]


def test_hashed_sources_agree_with_the_makefile():
    with open(os.path.join(REPO, "cosnet_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).replace("$(VARIANT_SRCS)", "").split()
    hashed = re.search(r"^HASHED := (.*)$", mk, re.M).group(1).replace("$(SRCS)", " ".join(srcs)).split()
    assert hashed == _native.HASHED_SOURCES
    head = "../../include/cosnet_hip_infer_head.h"
    i = hashed.index(head)
    assert hashed[i - 1] == "../../include/cosnet_hip_infer_fp8.h" and hashed[i + 1] == "common.h"
    assert hashed[-1] == "../../include/cosnet_hip_infer.h"
    assert re.search(r"^\$\(OBJDIR\)/conv\.o:.*cosnet_hip_infer_head\.h", mk, re.M)


def test_library_exports_the_head_symbols():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for n in HEAD:
        assert hasattr(lib, n), n
    assert _native.load().cn_conv_fwd_affine_add.argtypes[22] is ctypes.c_longlong


# ---- the command line ----------------------------------------------------------------------------------
def test_cli_refuses_split_reduce_without_the_bank(capsys):
    import test as test_cli
    with pytest.raises(SystemExit) as e:
        test_cli.get_arguments(["--dataset", "synthetic", "--split-reduce"])
    assert e.value.code == 2 and "--split-reduce" in capsys.readouterr().err
    for extra in ([], ["--fold-bn"], ["--dtype", "fp8", "--fp8-fold-bn"], ["--coatt", "mxfp8"], ["--dtype", "fp32"]):
        args = test_cli.get_arguments(["--dataset", "synthetic", "--feature-bank", "--split-reduce"] + extra)
        assert args.split_reduce
    assert not test_cli.get_arguments(["--dataset", "synthetic", "--feature-bank"]).split_reduce


# ---- the algebra -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, c, cout", [(3, 8, 6), (1, 4, 5), (3, 3, 2)])
def test_conv_over_a_concat_is_the_sum_of_the_convs_of_the_halves(k, c, cout):
    """fp64 on the CPU: conv(W, [a | b]) == conv(W[..., :C], a) + conv(W[..., C:], b) with the halves
    ops.weight_halves cuts from the forward operand [Cout][k][k][2C]."""
    g = torch.Generator().manual_seed(k * 100 + c)
    a = torch.randint(-4, 5, (2, c, 7, 5), generator=g).double()
    b = torch.randint(-4, 5, (2, c, 7, 5), generator=g).double()
    wt = torch.randint(-3, 4, (cout, 2 * c, k, k), generator=g).double()
    wf = wt.permute(0, 2, 3, 1).reshape(cout, k * k * 2 * c).contiguous()
    wz, wv = ops.weight_halves(wf, k)
    assert wz.is_contiguous() and wv.is_contiguous() and wz.shape == wv.shape == (cout, k * k * c)
    back = lambda h: h.view(cout, k, k, c).permute(0, 3, 1, 2)
    assert torch.equal(back(wz), wt[:, :c]) and torch.equal(back(wv), wt[:, c:])
    whole = F.conv2d(torch.cat([a, b], 1), wt, None, 1, k // 2)
    assert torch.equal(whole, F.conv2d(a, back(wz), None, 1, k // 2) + F.conv2d(b, back(wv), None, 1, k // 2))
    out = torch.full((2, cout, k * k * c), 99.0, dtype=torch.float64)       # filled in place
    z2, v2 = ops.weight_halves(wf, k, out=out)
    assert z2.data_ptr() == out.data_ptr() and torch.equal(z2, wz) and torch.equal(v2, wv)
    with pytest.raises(ValueError):
        ops.weight_halves(wf[:, :-1], k)


# ---- the generators' guard conditions ----------------------------------------------------------------------
def test_add_generators_meet_their_conditions():
    """Every comparison of test_gpu_conv_affine_add.py: the pre-activation (acc + bias + add) *
    scale + shift is exact in fp32 and below 2^24 with >= 10 % bf16 ties; after the ReLU >= 5 %
    ties and 40-60 % zeros (pytest -s prints the ranges)."""
    pre, post, zeros = [], [], []
    for label, ap in D.all_add_problems():
        a, b, z = A.verify_affine(ap)
        pre.append(a)
        if ap.act == 1:
            post.append(b)
            zeros.append(z)
        # the reference is the contract written out, row by row through the map
        m, cout = ap.pre.ref.shape
        j = torch.arange(m) // ap.add_rows
        r = torch.arange(m) % ap.add_rows
        f = torch.tensor(ap.fmap)[j]
        acc = (ap.pre.ref - ap.shift.view(1, -1)) / ap.scale.view(1, -1) - ap.bank[f, r]
        conv = ap.conv.outs["fwd"].ref
        assert (torch.equal(acc, D.rows_of(conv))
                or torch.equal(acc, D.rows_of(conv - ap.conv.bias.view(1, -1, 1, 1)))), label
    assert len(pre) >= 20
    print("ties before the activation %.1f-%.1f %%, after the ReLU %.1f-%.1f %%, zeros %.1f-%.1f %%" % (
        100 * min(pre), 100 * max(pre), 100 * min(post), 100 * max(post), 100 * min(zeros), 100 * max(zeros)))
    assert min(pre) >= A.MIN_TIES_PRE and min(post) >= A.MIN_TIES_RELU
    assert A.ZEROS[0] <= min(zeros) and max(zeros) <= A.ZEROS[1]


def test_the_map_of_the_generators_names_frames_the_bank_holds():
    ap = D.add_problem(D.CASE_64, 1, True)
    assert ap.fmap == [2, 0, 2] and ap.bank.shape[0] == D.BANK == 4 and ap.add_rows == 13 * 11
    assert D.add_problem(D.CASE_64, 1, True, "null").fmap == [0, 1, 2]
    assert D.add_problem(D.CASE_64, 1, True, "whole").add_rows == 3 * 13 * 11


# ---- refusals that need no device -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_cpu():
    return C.build_model(torch.bfloat16).eval()


def test_set_head_split_refusals_without_a_device(model_cpu):
    m = model_cpu
    assert m.head_split is None and m.set_head_split(False) is m
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.set_head_split()
    finally:
        m.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        m.set_head_split()      # a CPU model: no device to build the tables on
    assert m.head_split is None


def test_split_head_refusals_without_a_device(model_cpu):
    from cosnet_amd.inference import FeatureBank, segment_sequence
    m = model_cpu
    x, d = torch.zeros(2, 3, 33, 33), torch.zeros(2, 1, 33, 33)
    with pytest.raises(ValueError, match="head"):
        segment_sequence(m, x, d, [[1], [0]], head="both")
    feats = torch.zeros((2 * 9, 256), dtype=torch.bfloat16)
    bank = FeatureBank(feats, feats, feats, feats, (2, 3, 3), (33, 33))
    assert bank.partials is None
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="set_head_split"):
            m.head_a_indexed(bank, [0], [1], split=True)
        with pytest.raises(RuntimeError, match="set_head_split"):
            bank.reduce_partials(m)
        m.head_split = object()      # as set_head_split() leaves it
        try:
            with pytest.raises(ValueError, match="frame_chunk"):
                bank.reduce_partials(m, frame_chunk=0)
            m.fp8 = object()         # as set_fp8(True) leaves it
            try:
                with pytest.raises(RuntimeError, match="set_fp8"):
                    m.head_a_indexed(bank, [0], [1], split=True)
            finally:
                m.fp8 = None
            m.train()
            try:
                with pytest.raises(RuntimeError, match="eval"):
                    m.head_a_indexed(bank, [0], [1], split=True)
            finally:
                m.eval()
        finally:
            m.head_split = None
    with pytest.raises(RuntimeError, match="no_grad"):
        m.head_a_indexed(bank, [0], [1], split=True)      # grad enabled


def test_half_weight_cache_follows_the_weight(monkeypatch):
    """HalfWeightCache refreshes its copies in place when the weight's tag changed, and only then
    (WeightCache's rule); the launches are replaced by torch copies: no device needed."""
    calls = []

    def get(w, dtype, cin_pad=None, need_t=True):
        calls.append(w)
        return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(dtype).contiguous(), None

    monkeypatch.setattr(ops.WCACHE, "get", get)
    hc = ops.HalfWeightCache()
    w = torch.nn.Parameter(torch.randn(4, 6, 3, 3).contiguous(memory_format=torch.channels_last))
    with torch.no_grad():
        wz, wv = hc.get(w, torch.float32)
        assert len(calls) == 1 and torch.equal(wz.view(4, 3, 3, 3).permute(0, 3, 1, 2), w[:, :3])
        assert torch.equal(wv.view(4, 3, 3, 3).permute(0, 3, 1, 2), w[:, 3:])
        hc.get(w, torch.float32)
        assert len(calls) == 1                                     # nothing changed: no copy
        w.add_(1.0)                                                # in place: the version counter
        wz2, wv2 = hc.get(w, torch.float32)
        assert len(calls) == 2 and wz2.data_ptr() == wz.data_ptr() and wv2.data_ptr() == wv.data_ptr()
        assert torch.equal(wv2.view(4, 3, 3, 3).permute(0, 3, 1, 2), w[:, 3:])
