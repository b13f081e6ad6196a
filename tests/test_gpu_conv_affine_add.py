"""cn_conv_fwd_partial and cn_conv_fwd_affine_add (include/cosnet_hip_infer_head.h): the two
launches of a forward conv split by input channels -- bitwise, no tolerance.

The generators and the buffers are tests/test_gpu_exact_gemm.py's and tests/test_gpu_conv_affine.py's:
integer operands make the accumulator exact, the addend rows are integers in [-8, 8] looked up in a
bank of frames through a map, `scale` in {1/2, 1, 2} keeps the product exact and `shift` =
offset_bias puts the pre-activation values where bf16's spacing is >= 1, so a share of them are
exact ties.  The contract then reads bitwise: the stored value is ONE round-to-nearest-even
rounding of act(fma(acc + bias + add[map], scale, shift)) (bf16) or that value itself (fp32), and
the partial is the exact integer.  tests/test_cpu_head_split.py checks the generators' guard
conditions without a GPU.

The shapes are the smallest that can go wrong: 13 x 11 = 143 rows per block with 3 blocks
(M = 429: 128-row tiles and their staging passes straddle block boundaries), the map [2, 0, 2] into
a bank of 4 frames whose fourth frame, like everything around the bank, is NaN, a null map,
add_rows = M, Cout 64 / 256 / 72 (a ragged column tile), an addend view offset by one float (the
element-wise read), every tile launch_epi instantiates, both loaders the epilogue is instantiated
on, and the one fp32 shape that reaches the fp32 path's second tile (>= 384 blocks of 128 x 128).
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

import test_gpu_exact_gemm as E
from test_gpu_exact_gemm import (ROWPAD, ROWS_PAST, Out, bf, bound_of, conv_problem, f32, ints, offset_bias,
                                 operand, output, rows_of, same, untouched, wf_of)
from test_gpu_conv_affine import ACTS, EPI_TILES, PRELU_SLOPE, act_of, affine_scale, verify_affine

pytestmark = pytest.mark.gpu

# n, cin, h, w, cout, k, stride, pad, dil
CASE_256 = (3, 64, 13, 11, 256, 3, 1, 1, 1)     # the conv gather; two 128-column tiles
CASE_64 = (3, 64, 13, 11, 64, 3, 1, 1, 1)
CASE_DENSE = (3, 32, 9, 11, 72, 1, 1, 0, 1)     # the plain product; Cout = 72: a ragged column tile
ADD_CASES = [CASE_256, CASE_64, CASE_DENSE]
CASE_F32_TILE1 = (3, 32, 32, 64, 1024, 3, 1, 1, 1)   # fp32: 48 x 8 = 384 tiles of 128 x 128
CASE_CONV_G = (3, 32, 13, 11, 64, 3, 1, 1, 1)   # bf16: 32 channels per tap, K tiles straddle taps
STEM = (2, 8, 29, 31, 64, 7, 2, 3, 1)
BANK = 4
MAP = (2, 0, 2)
MODES = ("map", "null", "whole")


def add_problem(case, act, with_bias, mode="map", perm=MAP, seed=0):
    return _add_problem(case, act, with_bias, mode, tuple(perm), seed)


@functools.lru_cache(maxsize=None)
def _add_problem(case, act, with_bias, mode, perm, seed):
    """The exact pre-activation and stored values, as rows [M][Cout], of one conv with an addend on
    conv_problem(case)'s x, w and bias (never written).  mode "map": blocks of oh*ow rows take the
    frames `perm` of a bank of BANK frames; "null": block j takes frame j of a bank of n frames;
    "whole": one block of M rows."""
    n, cin, h, w, cout, k, s, p, d = case
    pr = conv_problem(case, E.ROUND, seed, False)
    sd = 100 * seed + 9000
    acc = pr.outs["fwd"].ref if with_bias else pr.outs["fwd"].ref - pr.bias.view(1, -1, 1, 1)
    acc = rows_of(acc)
    m = acc.shape[0]
    add_rows = m if mode == "whole" else pr.oh * pr.ow
    frames = BANK if mode == "map" else m // add_rows
    fmap = list(perm) if mode == "map" else list(range(frames))
    assert len(fmap) == m // add_rows
    bank = ints((frames, add_rows, cout), -8, 8, sd + 4)
    scale, shift = affine_scale(cout, sd + 1), offset_bias(cout, sd + 2)
    pre = (acc + bank[fmap].reshape(m, cout)) * scale.view(1, -1) + shift.view(1, -1)
    bound = 2 * (bound_of(k * k * cin, pr.x, pr.w, pr.bias if with_bias else None) + 8) + E.amax(shift)
    return SimpleNamespace(conv=pr, scale=scale, shift=shift, act=act, bank=bank, fmap=fmap,
                           add_rows=add_rows, mode=mode, pre=Out(pre, bound, step=0.5),
                           out=Out(act_of(pre, act), bound, step=0.5 * (PRELU_SLOPE if act == 2 else 1.0)))


def all_add_problems():
    """(label, problem) of every comparison of this file on the integer generators."""
    res = []
    for case in ADD_CASES:
        for act in ACTS:
            for with_bias in (False, True):
                res.append(("%s act %d bias %d" % (case, act, with_bias), add_problem(case, act, with_bias)))
    for mode in ("null", "whole"):
        res.append(("%s %s" % (CASE_64, mode), add_problem(CASE_64, 1, True, mode)))
    res.append(("%s permuted" % (CASE_64,), add_problem(CASE_64, 1, True, perm=(0, 2, 2))))
    res.append(("%s fp32 tile 1" % (CASE_F32_TILE1,), add_problem(CASE_F32_TILE1, 1, True)))
    res.append(("%s fp32" % (CASE_CONV_G,), add_problem(CASE_CONV_G, 1, True)))
    return res


def bank_operand(ap, dev, offset=0):
    """The bank as an fp32 [frames * add_rows][Cout] view in a NaN buffer (operand()'s layout, the
    view `offset` floats further right); in "map" mode its last frame -- which the map never names
    -- is NaN too."""
    rows = ap.bank.reshape(-1, ap.bank.shape[-1]).clone()
    if ap.mode == "map":
        rows[(BANK - 1) * ap.add_rows:] = float("nan")
    p, c = rows.shape
    buf = torch.full((p + ROWS_PAST, c + ROWPAD + 4), float("nan"), dtype=f32)
    buf[:p, ROWPAD + offset:ROWPAD + offset + c] = rows.to(f32)
    buf = buf.to(dev)
    return buf[:p, ROWPAD + offset:ROWPAD + offset + c]


def run_add(dev, dt, case, act, with_bias, mode="map", perm=MAP, offset=0, what="add"):
    ap = add_problem(case, act, with_bias, mode, perm)
    verify_affine(ap)
    pr = ap.conv
    n, cin, h, w, cout, k, s, p, d = case
    m = n * pr.oh * pr.ow
    ybuf, yv = output(m, cout, dt, dev)
    prelu = torch.tensor([PRELU_SLOPE], dtype=f32, device=dev) if act == 2 else None
    fmap = torch.tensor(ap.fmap, dtype=torch.int32, device=dev) if mode == "map" else None
    ops.conv_fwd_affine_add(operand(rows_of(pr.x), dt, dev), n, h, w, wf_of(pr.w, dt, dev), cout, k, s, p, d,
                            ap.scale.to(f32).to(dev), ap.shift.to(f32).to(dev), bank_operand(ap, dev, offset),
                            ap.add_rows, add_map=fmap, act=act, prelu=prelu,
                            bias=pr.bias.to(f32).to(dev) if with_bias else None, out=yv)
    torch.cuda.synchronize()
    label = "%s %s %s act %d bias %d %s offset %d" % (what, case, dt, act, with_bias, mode, offset)
    same(yv, ap.out.expect(dt), label)
    untouched(ybuf, m, cout, label)
    return yv


@pytest.fixture
def force_cfg():
    lib = nv.load()
    yield lib.cn_gemm_force_config
    lib.cn_gemm_force_config(-1)


# ---- cn_conv_fwd_partial ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", ADD_CASES + [CASE_CONV_G, STEM])
def test_conv_fwd_partial_is_the_exact_accumulator(cuda, dt, case):
    """y (fp32, whatever the operands) is the exact integer acc (+ bias); nothing outside the
    [M, Cout] view is touched.  Every loader: the plain product, both conv gathers."""
    n, cin, h, w, cout, k, s, p, d = case
    pr = conv_problem(case, E.ROUND, 0, False)
    m = n * pr.oh * pr.ow
    x, wf = operand(rows_of(pr.x), dt, cuda), wf_of(pr.w, dt, cuda)
    for with_bias in (False, True):
        out = pr.outs["fwd"] if with_bias else Out(pr.outs["fwd"].ref - pr.bias.view(1, -1, 1, 1),
                                                   pr.outs["fwd"].bound)
        E.verify(out)
        ybuf, yv = output(m, cout, f32, cuda)
        got, oh, ow = ops.conv_fwd_partial(x, n, h, w, wf, cout, k, s, p, d,
                                           bias=pr.bias.to(f32).to(cuda) if with_bias else None, out=yv)
        torch.cuda.synchronize()
        assert (oh, ow) == (pr.oh, pr.ow) and got.dtype == f32
        same(yv, rows_of(out.ref).to(f32), "partial %s %s bias %d" % (case, dt, with_bias))
        untouched(ybuf, m, cout, "partial %s" % (case,))


# ---- cn_conv_fwd_affine_add: the contract -------------------------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", ADD_CASES)
def test_conv_fwd_affine_add_exact(cuda, dt, case):
    """act 0 / 1 / 2, with and without a bias, the map [2, 0, 2] into a bank of 4 frames."""
    for act in ACTS:
        for with_bias in (False, True):
            run_add(cuda, dt, case, act, with_bias)


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("mode", ["null", "whole"])
def test_conv_fwd_affine_add_null_map_and_one_block(cuda, dt, mode):
    run_add(cuda, dt, CASE_64, 1, True, mode=mode)


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", [CASE_256, CASE_DENSE])
def test_conv_fwd_affine_add_reads_a_misaligned_addend_element_wise(cuda, dt, case):
    """The addend view one float off the 16-byte grid: no row takes the vector loads."""
    run_add(cuda, dt, case, 1, True, offset=1)
    run_add(cuda, dt, case, 2, False, offset=1)


@pytest.mark.parametrize("cfg", EPI_TILES)
def test_conv_fwd_affine_add_every_epilogue_tile(cuda, force_cfg, cfg):
    """Every tile launch_epi instantiates, on both loaders (M = 429 / 297: ragged rows; Cout = 72:
    ragged columns), blocks of 143 / 99 rows against tiles of 128 / 256."""
    force_cfg(cfg)
    run_add(cuda, bf, CASE_256, 1, True, what="tile %d" % cfg)
    run_add(cuda, bf, CASE_DENSE, 2, True, what="tile %d" % cfg)
    run_add(cuda, bf, CASE_DENSE, 0, False, offset=1, what="tile %d" % cfg)


def test_conv_fwd_affine_add_fp32_second_tile(cuda):
    """The fp32 path picks its 128 x 128 tile from 384 blocks on: M = 6144, Cout = 1024."""
    n, _, h, w, cout = CASE_F32_TILE1[:5]
    assert (n * h * w // 128) * (cout // 128) >= 384
    run_add(cuda, f32, CASE_F32_TILE1, 1, True)


def test_a_permuted_map_changes_the_result(cuda):
    """The map is read: [0, 2, 2] and [2, 0, 2] each give their own exact result, and differ."""
    for dt in (f32, bf):
        a = run_add(cuda, dt, CASE_64, 1, True, perm=(2, 0, 2))
        b = run_add(cuda, dt, CASE_64, 1, True, perm=(0, 2, 2))
        rows = 13 * 11
        assert not torch.equal(a[:rows], b[:rows]) and not torch.equal(a[rows:2 * rows], b[rows:2 * rows])
        assert torch.equal(a[2 * rows:], b[2 * rows:])


# ---- split equals concat ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf])
def test_split_equals_concat(cuda, dt):
    """Cin = 2 x 64 integer operands: conv_fwd_affine over [gz | v[map]] with the whole weight is
    bitwise conv_fwd_partial over the bank + conv_fwd_affine_add over gz with the halves
    (ops.weight_halves)."""
    n, c, h, w, cout = 3, 64, 13, 11, 64
    hw = h * w
    gz = ints((n * hw, c), -4, 4, 501)
    v = ints((BANK * hw, c), -4, 4, 502)
    wt = ints((cout, 2 * c, 3, 3), -3, 3, 503)
    scale, shift = affine_scale(cout, 504).to(f32).to(cuda), offset_bias(cout, 505).to(f32).to(cuda)
    fmap = torch.tensor(MAP, dtype=torch.int32)
    cat = torch.cat([gz, v.view(BANK, hw, c)[fmap.long()].reshape(n * hw, c)], 1)
    wf = wf_of(wt, dt, cuda)
    wz, wv = ops.weight_halves(wf, 3)
    assert wz.is_contiguous() and wv.is_contiguous() and wz.shape == wv.shape == (cout, 9 * c)
    for act in (0, 1):
        whole, _, _ = ops.conv_fwd_affine(operand(cat, dt, cuda), n, h, w, wf, cout, 3, 1, 1, 1, scale, shift, act=act)
        u, _, _ = ops.conv_fwd_partial(operand(v, dt, cuda), BANK, h, w, wv, cout, 3, 1, 1, 1)
        split, _, _ = ops.conv_fwd_affine_add(operand(gz, dt, cuda), n, h, w, wz, cout, 3, 1, 1, 1, scale, shift, u, hw,
                                              add_map=fmap.to(cuda), act=act)
        torch.cuda.synchronize()
        assert torch.isfinite(whole.float()).all()
        same(split, whole.cpu(), "split vs concat %s act %d" % (dt, act))


# ---- refusals -------------------------------------------------------------------------------------------
class Raw:
    """One valid raw call of cn_conv_fwd_affine_add on CASE_64 (bf16); call(**over) replaces
    arguments by name."""

    def __init__(self, dev):
        n, cin, h, w, cout, k, s, p, d = CASE_64
        pr = conv_problem(CASE_64, E.ROUND, 0, False)
        self.m = n * pr.oh * pr.ow
        self.x, self.wf = operand(rows_of(pr.x), bf, dev), wf_of(pr.w, bf, dev)
        _, self.y = output(self.m, cout, bf, dev)
        self.tab = torch.ones((cout + 4,), dtype=f32, device=dev)
        self.add = torch.zeros((BANK * pr.oh * pr.ow, cout), dtype=f32, device=dev)
        self.map = torch.tensor(MAP + (0,), dtype=torch.int32, device=dev)
        self.args = dict(dtype=nv.DT_BF16, x=self.x.data_ptr(), ldx=ops.ld(self.x), N=n, H=h, W=w, Cin=cin,
                         w=self.wf.data_ptr(), Cout=cout, KH=k, KW=k, stride=s, pad=p, dil=d, bias=None,
                         y=self.y.data_ptr(), ldy=ops.ld(self.y), OH=pr.oh, OW=pr.ow, scale=self.tab.data_ptr(),
                         shift=self.tab.data_ptr(), add=self.add.data_ptr(), lda=cout, add_map=self.map.data_ptr(),
                         add_rows=pr.oh * pr.ow, act=0, prelu=None)
        assert list(self.args) == nv._head_extension_signatures()["cn_conv_fwd_affine_add"][2][:-1]

    def call(self, **over):
        a = dict(self.args, **over)
        assert set(a) == set(self.args)
        return nv.call("cn_conv_fwd_affine_add", *a.values(), nv.stream())


@pytest.fixture(scope="module")
def raw(cuda):
    return Raw(cuda)


def test_the_valid_raw_call_runs(raw):
    raw.call()
    torch.cuda.synchronize()
    assert torch.isfinite(raw.y.float()).all()


@pytest.mark.parametrize("over", [dict(add=None), dict(add_rows=0), dict(add_rows=-143), dict(add_rows=100),
                                  dict(lda=63)], ids=["add-null", "rows-0", "rows-negative", "rows-not-dividing-M",
                                                      "lda-below-Cout"])
def test_affine_add_shape_refusals(raw, over):
    with pytest.raises(nv.NativeError, match="shape"):
        raw.call(**over)


@pytest.mark.parametrize("arg", ["scale", "shift", "add_map"])
def test_affine_add_alignment_refusals(raw, arg):
    off = raw.tab.data_ptr() + 4 if arg != "add_map" else raw.map.data_ptr() + 2
    with pytest.raises(nv.NativeError, match="alignment"):
        raw.call(**{arg: off})


@pytest.mark.parametrize("over", [dict(dtype=2), dict(dtype=7), dict(act=3), dict(act=-1), dict(act=2)],
                         ids=["dtype-2", "dtype-7", "act-3", "act-negative", "prelu-without-slope"])
def test_affine_add_unsupported_refusals(raw, over):
    with pytest.raises(nv.NativeError, match="unsupported"):
        raw.call(**over)


def test_affine_add_refuses_what_is_not_instantiated(cuda, force_cfg):
    """The per-thread-pointer gather (32 bf16 channels per tap) and a forced tile without the
    epilogue are refused, not replaced; the same shape in fp32 (32 channels = one K tile) runs."""
    with pytest.raises(nv.NativeError, match="unsupported"):
        run_add(cuda, bf, CASE_CONV_G, 1, True)
    run_add(cuda, f32, CASE_CONV_G, 1, True)
    force_cfg(0)
    with pytest.raises(nv.NativeError, match="unsupported"):
        run_add(cuda, bf, CASE_64, 1, True)


def test_partial_refuses_other_dtypes(raw):
    a = list(raw.args.values())[:19]
    u = torch.empty((raw.m, 64), dtype=f32, device=raw.add.device)
    a[15], a[16] = u.data_ptr(), 64
    for code in (2, 7):
        with pytest.raises(nv.NativeError, match="unsupported"):
            nv.call("cn_conv_fwd_partial", code, *a[1:], nv.stream())
    nv.call("cn_conv_fwd_partial", *a, nv.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(u).all()
