"""The status codes with which the convolution entry points (csrc/conv.hip) refuse a call.

Every case here is refused by the host code BEFORE its first launch, so nothing runs on the device:
the tensors only have to be real allocations large enough for the stated shapes.  What is pinned
is the code (nv.call turns it into the words `shape`, `alignment`, `unsupported`) and, where two
things are wrong at once, which check comes first.  That includes the contract's present
asymmetries: only the fp8 input gradient checks the output size, and a null fp8 scale state in
cn_conv_wgrad_fp8 is reported as an alignment error.

Shapes: N = 1, 4 x 4 pixels, 16 or 32 channels; the split-K weight gradient takes 32 x 32 pixels,
the smallest square at which the bf16 plan splits.
"""
import ctypes
import types

import pytest
import torch

from cosnet_amd import _native as nv

pytestmark = pytest.mark.gpu

BF = nv.DT_BF16
N, H, W = 1, 4, 4
SHAPE, ALIGN, UNSUPPORTED = r"shape \(-1\)", r"alignment \(-2\)", r"unsupported \(-3\)"


@pytest.fixture(scope="module")
def t(cuda):
    """a: any bf16 operand or output, q: any fp8 operand, f: any fp32 output, workspace, statistic
    or scale state.  Each covers the largest shape of this file."""
    return types.SimpleNamespace(
        a=torch.zeros((1024, 32), dtype=torch.bfloat16, device=cuda),
        q=torch.zeros((1024, 32), dtype=torch.uint8, device=cuda),
        f=torch.zeros((65536,), dtype=torch.float32, device=cuda))


def refused(words, name, *args):
    with pytest.raises(nv.NativeError, match=words):
        nv.call(name, *args, nv.stream())


def arr(g, p):
    """Host array of g copies of pointer p (None: null)."""
    return (ctypes.c_void_p * g)(*[p] * g)


def fwd(x, w, y, cin=16, cout=16, k=1, stride=1, pad=0, dil=1, oh=H, ow=W, dt=None):
    """Arguments of the forward entries up to OW (the fp8 ones take no dtype)."""
    head = () if dt is None else (dt,)
    return head + (x.data_ptr(), cin, N, H, W, cin, w.data_ptr(), cout, k, k, stride, pad, dil, None,
                   y.data_ptr(), cout, oh, ow)


def bn_tail(t, nseg=1, ws=True):
    f = t.f.data_ptr()
    return (nseg, f if ws else None, f, f, f, f, 0.1, 1e-5)


def wgrad_grouped(t, g, dt=BF):
    """Arguments of cn_conv_wgrad_grouped up to dws, host arrays of max(g, 1) entries."""
    n = max(g, 1)
    return (dt, g, arr(n, t.a.data_ptr()), 16, N, H, W, 16, arr(n, t.a.data_ptr()), 16, H, W, 16, 1, 1,
            1, 0, 1, arr(n, t.f.data_ptr()))


def wgrad_fp8(t, g, x_state=True):
    n = max(g, 1)
    q, f = t.q.data_ptr(), t.f.data_ptr()
    return (g, arr(n, q), 16, N, H, W, 16, arr(n, q), 16, H, W, 16, 1, 1, 1, 0, 1, arr(n, f),
            arr(n, f if x_state else None), arr(n, f), f, t.f.numel())


# ---- channels that are no multiple of the 16-byte vector -----------------------------------------
def test_fwd_cin_not_a_vector_multiple(t):
    refused(ALIGN, "cn_conv_fwd", *fwd(t.a, t.a, t.a, cin=12, dt=BF))


def test_fwd_ws_without_workspace_falls_back_to_fwd(t):
    refused(ALIGN, "cn_conv_fwd_ws", *fwd(t.a, t.a, t.a, cin=12, dt=BF), None, 0)


def test_fwd_bn_cin_not_a_vector_multiple(t):
    refused(ALIGN, "cn_conv_fwd_bn", *fwd(t.a, t.a, t.a, cin=12, dt=BF), *bn_tail(t))


def test_fwd_fp8_cin_multiple_of_8_only(t):
    f = t.f.data_ptr()
    refused(ALIGN, "cn_conv_fwd_fp8", *fwd(t.q, t.q, t.a, cin=8), f, f)


def test_wgrad_cin_not_a_vector_multiple(t):
    a, f = t.a.data_ptr(), t.f.data_ptr()
    refused(ALIGN, "cn_conv_wgrad", BF, a, 12, N, H, W, 12, a, 16, H, W, 16, 1, 1, 1, 0, 1, f, f)


# ---- an output size that is not the convolution's ------------------------------------------------
def test_fwd_wrong_oh(t):
    refused(SHAPE, "cn_conv_fwd", *fwd(t.a, t.a, t.a, oh=H + 1, dt=BF))
    refused(SHAPE, "cn_conv_fwd", *fwd(t.a, t.a, t.a, k=3, pad=1, oh=H - 1, dt=BF))


def test_fwd_bn_wrong_oh(t):
    refused(SHAPE, "cn_conv_fwd_bn", *fwd(t.a, t.a, t.a, oh=H + 1, dt=BF), *bn_tail(t))


def dgrad_fp8(t, cout=16, oh=H):
    f = t.f.data_ptr()
    return (t.q.data_ptr(), cout, N, oh, W, cout, t.q.data_ptr(), 16, 1, 1, 0, 1, t.a.data_ptr(), 16, H,
            W, 0, f, f)


def test_dgrad_fp8_wrong_oh(t):
    refused(SHAPE, "cn_conv_dgrad_fp8", *dgrad_fp8(t, oh=H + 1))


def test_alignment_is_checked_before_the_output_size(t):
    refused(ALIGN, "cn_conv_fwd", *fwd(t.a, t.a, t.a, cin=12, oh=H + 1, dt=BF))
    refused(ALIGN, "cn_conv_fwd_bn", *fwd(t.a, t.a, t.a, cin=12, oh=H + 1, dt=BF), *bn_tail(t))
    refused(ALIGN, "cn_conv_dgrad_fp8", *dgrad_fp8(t, cout=8, oh=H + 1))


# ---- BN-statistics epilogues -----------------------------------------------------------------------
def test_fwd_bn_segments_must_divide_the_rows(t):
    refused(SHAPE, "cn_conv_fwd_bn", *fwd(t.a, t.a, t.a, dt=BF), *bn_tail(t, nseg=3))


def test_fwd_bn_needs_its_workspace(t):
    refused(SHAPE, "cn_conv_fwd_bn", *fwd(t.a, t.a, t.a, dt=BF), *bn_tail(t, ws=False))


def test_dgrad_bn_needs_its_workspace(t):
    a, f = t.a.data_ptr(), t.f.data_ptr()
    refused(SHAPE, "cn_conv_dgrad_bn", BF, a, 16, N, H, W, 16, a, 16, 1, 1, 0, 1, a, 16, H, W, a, 16, f,
            f, f, f, f, f, None)


# ---- input gradients the kernel does not cover -----------------------------------------------------
def dgrad(t, k, stride, oh, ow):
    a = t.a.data_ptr()
    return (BF, a, 16, N, oh, ow, 16, a, 16, k, k, stride, k // 2, 1, a, 16, H, W, 0)


def test_dgrad_stride_3(t):
    refused(UNSUPPORTED, "cn_conv_dgrad", *dgrad(t, 1, 3, 2, 2))


def test_dgrad_3x3_stride_2(t):
    refused(UNSUPPORTED, "cn_conv_dgrad", *dgrad(t, 3, 2, 2, 2))


# ---- weight gradients ------------------------------------------------------------------------------
def test_wgrad_grouped_empty_group(t):
    refused(SHAPE, "cn_conv_wgrad_grouped", *wgrad_grouped(t, 0))
    refused(SHAPE, "cn_conv_wgrad_grouped_ws", *wgrad_grouped(t, 0), t.f.data_ptr(), t.f.numel())


def test_wgrad_fp8_empty_group(t):
    refused(SHAPE, "cn_conv_wgrad_fp8", *wgrad_fp8(t, 0))


def test_wgrad_fp8_null_state_is_an_alignment_error(t):
    refused(ALIGN, "cn_conv_wgrad_fp8", *wgrad_fp8(t, 1, x_state=False))


def test_wgrad_split_needs_its_workspace(t):
    hw = 32
    assert nv.query("cn_conv_wgrad_workspace_floats", BF, N, hw, hw, 16, 1, 1, 16) > 0
    a = t.a.data_ptr()
    refused(SHAPE, "cn_conv_wgrad", BF, a, 16, N, hw, hw, 16, a, 16, hw, hw, 16, 1, 1, 1, 0, 1,
            t.f.data_ptr(), None)
