"""The weight-stationary persistent GEMM (csrc/gemm_ws.hip) against the generic implicit-GEMM
kernel it replaces for the shallow-K 1x1 products.

Every eligible problem is routed to it with cn_gemm_ws_mode(2) (and 3: one M walker per XCD, so a
block walks dozens of tiles and the A ring wraps many times).  Its results must be BITWISE those
of the generic kernel -- the shape heuristic's tile and the forced configurations 10 (256x256) and
11 (128x128) -- for plain stores (C pre-filled with NaN) and read-add-store (random old C), with
row strides wider than the rows and sentinel rows / columns around C that must stay untouched.
Shapes: every supported K, N with whole and partial last column slices, M of one tile (most
blocks idle), a partial tile, and an odd M near 20 000 (unequal tile counts per block).
"""
import functools

import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

import test_gpu_kernels as K

pytestmark = pytest.mark.gpu

KS = [64, 128, 256, 512]
NS = [256, 328]
MS = [64, 200, 20001]
PAD = 8          # lda = K + PAD, ldb = K + PAD, ldc = N + PAD (rows stay 16-byte aligned)
ROWS_PAST = 3    # sentinel rows past M
SENTINEL = 7.0
bf = torch.bfloat16


@pytest.fixture
def ws():
    """Sets the routing mode (and the forced tile configuration) for one launch; restores both."""
    lib = nv.load()
    prev = lib.cn_gemm_ws_mode(1)

    def set_mode(mode, cfg=-1):
        assert lib.cn_gemm_ws_mode(mode) >= 0
        assert lib.cn_gemm_force_config(cfg) > cfg
    yield set_mode
    lib.cn_gemm_force_config(-1)
    lib.cn_gemm_ws_mode(prev)


def ws_launches():
    return int(nv.load().cn_gemm_ws_launches())


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == bf else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def problem(m, n, k):
    """Operands (shared by the tests of one shape, never written): A [m, k + PAD], B [n, k + PAD],
    the old C [m + ROWS_PAST, n + PAD] with sentinels outside [m, n], and the fp64 product."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * k + n + m)
    a = torch.randn((m, k + PAD), generator=g).to(bf).to(dev)
    b = (torch.randn((n, k + PAD), generator=g) * (2.0 / k) ** 0.5).to(bf).to(dev)
    old = torch.randn((m + ROWS_PAST, n + PAD), generator=g).to(bf).to(dev)
    old[m:, :] = SENTINEL
    old[:, n:] = SENTINEL
    ref = a[:, :k].double() @ b[:, :k].double().t()
    return a, b, old, ref


def launch(m, n, k, c_mode):
    a, b, old, _ = problem(m, n, k)
    c = old.clone()
    if c_mode == 0:
        c[:m, :n] = float("nan")
    ops.gemm(a, b, m, n, k, lda=k + PAD, ldb=k + PAD, out=c, ldc=n + PAD, c_mode=c_mode)
    return c


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_bitwise_equal_to_generic_kernel(cuda, ws, m, n, k):
    _, _, old, ref = problem(m, n, k)
    for c_mode in (0, 2):
        want = []
        for cfg in (-1, 10, 11):
            ws(0, cfg)
            want.append(launch(m, n, k, c_mode))
        assert same_bits(want[0], want[1]) and same_bits(want[0], want[2])
        for mode in (2, 3):
            ws(mode)
            before = ws_launches()
            got = launch(m, n, k, c_mode)
            torch.cuda.synchronize()
            assert ws_launches() == before + 1   # the new kernel ran
            # sentinels untouched
            assert same_bits(got[m:, :], old[m:, :]) and same_bits(got[:, n:], old[:, n:])
            assert not torch.isnan(got[:m, :n]).any()
            assert same_bits(got, want[0]), (m, n, k, c_mode, mode)
        # accuracy against fp64 with the 1x1 conv cases' tolerance
        full = ref + (old[:m, :n].double() if c_mode == 2 else 0)
        K.close(got[:m, :n], full, bf)


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("c_mode", [0, 2])
def test_repeated_launches_are_deterministic(cuda, ws, mode, c_mode):
    """A fragment read racing an LDS-DMA fill, or an old-C register read before its load landed,
    shows up as run-to-run differences."""
    ws(mode)
    outs = [launch(20001, 328, 256, c_mode) for _ in range(6)]
    torch.cuda.synchronize()
    for y in outs[1:]:
        assert same_bits(y, outs[0])


def test_ineligible_problems_take_the_generic_path(cuda, ws):
    """Under mode 2 everything the new kernel does not cover gives the generic path's bits."""
    g = torch.Generator().manual_seed(5)
    m, n = 300, 256
    a = torch.randn((m, 256), generator=g).to(bf).to(cuda)
    b = (torch.randn((n, 256), generator=g) * 0.1).to(bf).to(cuda)
    bias = torch.randn((n,), generator=g).to(cuda)
    a96, b96 = a[:, :96].contiguous(), b[:, :96].contiguous()
    gemms = [
        lambda: ops.gemm(a96, b96, m, n, 96, lda=96, ldb=96),
        lambda: ops.gemm(a, b, m, n, 256, lda=256, ldb=256, bias=bias),
        lambda: ops.gemm(a, b, m, n, 256, lda=256, ldb=256, alpha=0.5),
        lambda: ops.gemm(a.float(), b.float(), m, n, 256, lda=256, ldb=256),
    ]
    # a 3x3 conv and a stride-2 1x1 dgrad
    nimg, h, w = 2, 13, 11
    x = torch.randn((nimg * h * w, 64), generator=g).to(bf).to(cuda)
    wp = (torch.randn((128, 64, 3, 3), generator=g) * 0.05).to(cuda).contiguous(memory_format=torch.channels_last)
    wf3, _ = ops.WCACHE.get(wp, bf)
    wp1 = (torch.randn((128, 256, 1, 1), generator=g) * 0.05).to(cuda).contiguous(memory_format=torch.channels_last)
    _, wt1 = ops.WCACHE.get(wp1, bf)
    oh, ow = ops.out_hw(h, w, 1, 2, 0, 1)
    dy = torch.randn((nimg * oh * ow, 128), generator=g).to(bf).to(cuda)
    gemms.append(lambda: ops.conv_fwd(x, nimg, h, w, wf3, 128, 3, 1, 1, 1)[0])
    gemms.append(lambda: ops.conv_dgrad(dy, nimg, oh, ow, wt1, 256, 1, 2, 0, 1, h, w))
    for i, f in enumerate(gemms):
        ws(0)
        want = f()
        ws(2)
        before = ws_launches()
        got = f()
        torch.cuda.synchronize()
        assert ws_launches() == before, i
        assert same_bits(got, want), i


def test_conv_level(cuda, ws):
    """1x1 conv forward / dgrad (plain and accumulating) through the new kernel: the kernel-parity
    case against fp64, and the generic kernel's bits on a bias-free forward and both dgrads."""
    ws(2)
    K.test_conv_fwd_dgrad_wgrad(cuda, bf, (2, 64, 13, 11, 128, 1, 1, 0, 1))
    g = torch.Generator().manual_seed(9)
    nimg, h, w, cin, cout = 3, 17, 19, 328, 128   # forward K = 328 is not covered; dgrad K = 128 is
    p = nimg * h * w
    dy = torch.randn((p, cout), generator=g).to(bf).to(cuda)
    dx0 = torch.randn((p, cin), generator=g).to(bf).to(cuda)
    wp = (torch.randn((cout, cin, 1, 1), generator=g) * 0.1).to(cuda).contiguous(memory_format=torch.channels_last)
    _, wtt = ops.WCACHE.get(wp, bf)
    # the forward of the transposed shape: 128 -> 328 channels
    wq = (torch.randn((cin, cout, 1, 1), generator=g) * 0.1).to(cuda).contiguous(memory_format=torch.channels_last)
    wfq, _ = ops.WCACHE.get(wq, bf)
    res = {}
    before = ws_launches()
    for mode in (0, 2):
        ws(mode)
        res[mode] = (ops.conv_fwd(dy, nimg, h, w, wfq, cin, 1, 1, 0, 1)[0],
                     ops.conv_dgrad(dy, nimg, h, w, wtt, cin, 1, 1, 0, 1, h, w),
                     ops.conv_dgrad(dy, nimg, h, w, wtt, cin, 1, 1, 0, 1, h, w, out=dx0.clone(), accumulate=True))
    torch.cuda.synchronize()
    assert ws_launches() == before + 3
    for want, got in zip(res[0], res[2]):
        assert same_bits(got, want)
    assert not same_bits(res[2][1], res[2][2])   # the accumulating dgrad did add
