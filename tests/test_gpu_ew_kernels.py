"""Direct parity of the memory-bound helpers (ew.hip, fp8.hip) against plain fp64 / bitwise
references, at the sizes where their loops change shape: one row, one chunk, a partly filled
block, more than one row split, the grid caps, and channel-slice views of a wider buffer.

Every reduction is checked twice.  Integer data drawn from {-1, 0, 1}: every fp32 partial sum
is an exact integer in any order, so the result must EQUAL the fp64 reference (one dropped row
or chunk changes it).  Real data: the usual relative tolerance, and two launches must agree
bitwise (the kernels claim fixed-order sums).
"""
import math

import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import fp8 as fp8mod
from cosnet_amd import ops

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}
DTS = [torch.float32, torch.bfloat16]
SENT = 123.0   # sentinel of pre-filled outputs (exact in bf16)


def vec(dt):
    return 8 if dt == torch.bfloat16 else 4


def close(got, ref, dt, scale=None):
    got = got.double().cpu()
    ref = ref.double().cpu()
    s = scale if scale is not None else max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item() / s
    assert err <= TOL[dt], "rel err %.3g > %.3g" % (err, TOL[dt])
    return err


def rnd(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dt).double()


def ints(shape, seed):
    """{-1, 0, 1}: exact in bf16 and fp32, and so is every partial sum of them in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, shape, generator=g).double()


def sliced(vals, dt, dev, fill=SENT):
    """vals [P, C] (fp64, CPU) as the column slice [V, V + C) of a buffer with ld = C + 3 V
    whose other columns hold `fill`.  Returns (buffer, view)."""
    p, c = vals.shape
    v = vec(dt)
    buf = torch.full((p, c + 3 * v), fill, dtype=dt, device=dev)
    view = buf[:, v:v + c]
    view.copy_(vals.to(dt))
    return buf, view


def outside_unchanged(buf, c, dt, fill=SENT):
    v = vec(dt)
    return bool((buf[:, :v] == fill).all()) and bool((buf[:, v + c:] == fill).all())


# ---- cn_avgpool ------------------------------------------------------------------------------
def _avgpool_cases(dt):
    v = vec(dt)
    # n, hw, c, row splits.  (3, 257, 520): two splits of 129 rows and a partly filled column
    # block.  (300, 769, v): ceil(769 / 256) = 4 splits x 300 images > 1024 blocks, cut to 3.
    # (1025, 3, v): 1024 / 1025 blocks per image = 0 splits, clamped to 1.
    return [(2, 1, v, 1), (3, 257, 520, 2), (300, 769, v, 3), (1025, 3, v, 1)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", range(4))
def test_avgpool(cuda, dt, case):
    n, hw, c, splits = _avgpool_cases(dt)[case]
    nws = int(nv.query("cn_avgpool_workspace_floats", nv.dtype_code(dt), n, hw, c))
    assert nws == splits * n * c
    if case == 2:   # really capped
        assert nws / (n * c) < math.ceil(hw / 256)
    # integers, scale 1: exact (bf16 output exact while |sum| <= 256)
    xi = ints((n * hw, c), 100 + case)
    ref = xi.view(n, hw, c).sum(1)
    assert ref.abs().max().item() <= 256
    out = torch.full((n, c), SENT, dtype=dt, device=cuda)
    ops.avgpool(xi.to(dt).to(cuda), n, hw, 1.0, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.to(dt))
    # real data, scale 1 / hw
    xr = rnd((n * hw, c), dt, 110 + case)
    xg = xr.to(dt).to(cuda)
    o1 = ops.avgpool(xg, n, hw, 1.0 / hw, torch.empty((n, c), dtype=dt, device=cuda))
    o2 = ops.avgpool(xg, n, hw, 1.0 / hw, torch.empty((n, c), dtype=dt, device=cuda))
    torch.cuda.synchronize()
    close(o1, xr.view(n, hw, c).mean(1), dt)
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("dt", DTS)
def test_avgpool_aspp_backward_slice(cuda, dt):
    """The ASPP backward call: the first 512 channels of an ld-2560 buffer, scale 1.0; the other
    2048 columns hold values that would wreck the sums if a row stride were mistaken."""
    n, hw, c, ldw = 2, 400, 512, 2560
    xi = ints((n * hw, c), 120)
    ref = xi.view(n, hw, c).sum(1)
    assert ref.abs().max().item() <= 256
    wide = torch.full((n * hw, ldw), 1000.0, dtype=dt, device=cuda)
    wide[:, :c].copy_(xi.to(dt))
    out = ops.avgpool(wide[:, :c], n, hw, 1.0, torch.full((n, c), SENT, dtype=dt, device=cuda))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.to(dt))
    xr = rnd((n * hw, c), dt, 121)
    wide[:, :c].copy_(xr.to(dt))
    o1 = ops.avgpool(wide[:, :c], n, hw, 1.0, torch.empty((n, c), dtype=dt, device=cuda))
    o2 = ops.avgpool(wide[:, :c], n, hw, 1.0, torch.empty((n, c), dtype=dt, device=cuda))
    torch.cuda.synchronize()
    close(o1, xr.view(n, hw, c).sum(1), dt)
    assert torch.equal(o1, o2)


# ---- cn_bcast_rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_bcast_rows(cuda, dt):
    v = vec(dt)
    n, hw, c = 3, 37, 9 * v
    src = rnd((n, c), dt, 130)
    sg = src.to(dt).to(cuda)
    buf, dst = sliced(torch.zeros((n * hw, c), dtype=torch.float64), dt, cuda)
    dst.fill_(SENT)
    nv.call("cn_bcast_rows", ops.dtc(sg), sg.data_ptr(), n, hw, c, 1.0, dst.data_ptr(), ops.ld(dst), 0,
            nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src.to(dt).repeat_interleave(hw, dim=0))
    assert outside_unchanged(buf, c, dt)
    # accumulate onto a random destination with the average pool's backward scale
    d0 = rnd((n * hw, c), dt, 131)
    ref = d0 + src.repeat_interleave(hw, dim=0) / hw
    res = []
    for _ in range(2):
        buf, dst = sliced(d0, dt, cuda)
        nv.call("cn_bcast_rows", ops.dtc(sg), sg.data_ptr(), n, hw, c, 1.0 / hw, dst.data_ptr(),
                ops.ld(dst), 1, nv.stream())
        torch.cuda.synchronize()
        assert outside_unchanged(buf, c, dt)
        res.append(dst.clone())
    close(res[0], ref, dt)
    assert torch.equal(res[0], res[1])


# ---- cn_colsum -------------------------------------------------------------------------------
def _colsum_check(cuda, dt, p, c, seed, strided):
    def put(vals):
        if strided:
            return sliced(vals, dt, cuda, fill=1000.0)[1]
        return vals.to(dt).to(cuda)
    xi = ints((p, c), seed)
    out = ops.colsum(put(xi), out=torch.full((c,), SENT, dtype=torch.float32, device=cuda))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), xi.sum(0).float())
    xr = rnd((p, c), dt, seed + 1)
    xg = put(xr)
    o1, o2 = ops.colsum(xg), ops.colsum(xg)
    torch.cuda.synchronize()
    # the inputs are exact in dt and the sums fp32 for both dtypes: the fp32 bound for both
    close(o1, xr.sum(0), torch.float32)
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("p", [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("wide", [False, True])
def test_colsum(cuda, dt, p, wide):
    _colsum_check(cuda, dt, p, 520 if wide else vec(dt), 140 + p, False)


@pytest.mark.parametrize("dt", DTS)
def test_colsum_row_block_cap(cuda, dt):
    """P > 256 * 64: the row-block count is capped at 256 and every block strides further."""
    _colsum_check(cuda, dt, 16450, 8, 150, False)


@pytest.mark.parametrize("dt", DTS)
def test_colsum_strided(cuda, dt):
    _colsum_check(cuda, dt, 257, 520, 152, True)


# ---- cn_sum_rows / cn_mean_rows --------------------------------------------------------------
@pytest.mark.parametrize("nrows", [1, 2, 3, 4, 5, 15, 16, 17, 29])
def test_sum_rows(cuda, nrows):
    """colreduce_k: the 16-row unrolled loop runs while b + 12 < nb, then a 4-row tail."""
    for c in (1, 63, 64, 65, 130):
        xi = ints((nrows, c), 160 + c)
        out = torch.full((c + 4,), SENT, dtype=torch.float32, device=cuda)
        xg = xi.float().to(cuda)
        nv.call("cn_sum_rows", xg.data_ptr(), nrows, c, out.data_ptr(), nv.stream())
        torch.cuda.synchronize()
        assert torch.equal(out[:c].cpu(), xi.sum(0).float()), (nrows, c)
        assert bool((out[c:] == SENT).all())
        xr = rnd((nrows, c), torch.float32, 161 + c)
        xg = xr.float().to(cuda)
        o = [torch.empty((c,), dtype=torch.float32, device=cuda) for _ in range(2)]
        for t in o:
            nv.call("cn_sum_rows", xg.data_ptr(), nrows, c, t.data_ptr(), nv.stream())
        torch.cuda.synchronize()
        close(o[0], xr.sum(0), torch.float32)
        assert torch.equal(o[0], o[1])


@pytest.mark.parametrize("nrows", [1, 2, 5])
@pytest.mark.parametrize("c", [1, 257, 97 * 97])
def test_mean_rows_is_the_sequential_fp32_mean(cuda, nrows, c):
    """The kernel's contract is the reference's running fp32 `sum += x` then `/ n`: bitwise the
    same loop in torch fp32 on the CPU."""
    x = rnd((nrows, c), torch.float32, 170 + nrows).float()
    s = x[0].clone()
    for r in range(1, nrows):
        s += x[r]
    ref = s / torch.tensor(float(nrows), dtype=torch.float32)
    xg = x.to(cuda)
    out = torch.full((c + 4,), SENT, dtype=torch.float32, device=cuda)
    nv.call("cn_mean_rows", xg.data_ptr(), nrows, c, out.data_ptr(), nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:c].cpu(), ref)
    assert bool((out[c:] == SENT).all())


# ---- cn_scale / cn_scale_dev -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3])
def test_scale_and_scale_dev(cuda, n):
    """Bitwise an fp32 multiply; the last size exceeds the grid cap (grid-stride loop)."""
    x = rnd((n,), torch.float32, 180).float()
    s = torch.tensor(0.37, dtype=torch.float32)
    ref = x * s
    buf = torch.full((n + 8,), SENT, dtype=torch.float32, device=cuda)
    buf[:n].copy_(x)
    nv.call("cn_scale", buf.data_ptr(), n, s.item(), nv.stream())
    out = torch.full((n + 8,), SENT, dtype=torch.float32, device=cuda)
    xg, sg = x.to(cuda), s.reshape(1).to(cuda)
    nv.call("cn_scale_dev", xg.data_ptr(), n, sg.data_ptr(), out.data_ptr(), nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(buf[:n].cpu(), ref) and bool((buf[n:] == SENT).all())
    assert torch.equal(out[:n].cpu(), ref) and bool((out[n:] == SENT).all())
    assert torch.equal(xg.cpu(), x)


def test_scale_of_nothing_is_a_no_op(cuda):
    buf = torch.full((16,), SENT, dtype=torch.float32, device=cuda)
    nv.call("cn_scale", buf.data_ptr(), 0, 2.0, nv.stream())
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- cn_count_ge -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4095, 4097, 256 * 256 * 16 + 7])
def test_count_ge(cuda, n):
    g = torch.Generator().manual_seed(190)
    x = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (n,), generator=g)]   # some AT the threshold
    for vals, want in ((x, int((x >= 0.5).sum())), (torch.full((n,), 0.25), 0), (torch.full((n,), 0.5), n)):
        cnt = torch.full((1,), -0x123456789, dtype=torch.int64, device=cuda)   # the kernel zeroes it
        vg = vals.to(cuda)
        nv.call("cn_count_ge", vg.data_ptr(), n, 0.5, cnt.data_ptr(), nv.stream())
        torch.cuda.synchronize()
        assert cnt.item() == want


# ---- cn_rowdot / cn_rowdot_seg ---------------------------------------------------------------
def _rowdot(cuda, dt, a, b, p, c, seg=None, seg_ld=None):
    """a as a slice of a wider buffer, b contiguous (different row strides)."""
    ag = sliced(a, dt, cuda, fill=1000.0)[1]
    bg = b.to(dt).to(cuda)
    assert ops.ld(ag) != ops.ld(bg)
    if seg is None:
        out = torch.full((p + 8,), SENT, dtype=torch.float32, device=cuda)
        nv.call("cn_rowdot", ops.dtc(ag), ag.data_ptr(), ops.ld(ag), bg.data_ptr(), ops.ld(bg), p, c,
                out.data_ptr(), nv.stream())
    else:
        out = torch.full((p // seg * seg_ld,), SENT, dtype=torch.float32, device=cuda)
        nv.call("cn_rowdot_seg", ops.dtc(ag), ag.data_ptr(), ops.ld(ag), bg.data_ptr(), ops.ld(bg), p, c,
                seg, seg_ld, out.data_ptr(), nv.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("p", [1, 3, 4, 5, 130])
def test_rowdot(cuda, dt, p):
    v = vec(dt)
    for c in (v, 256, 65 * v):   # 65 chunks: lane 0 takes a second one
        a, b = ints((p, c), 200 + c), ints((p, c), 201 + c)
        out = _rowdot(cuda, dt, a, b, p, c)
        assert torch.equal(out[:p].cpu(), (a * b).sum(1).float()), (p, c)
        assert bool((out[p:] == SENT).all())
        a, b = rnd((p, c), dt, 202 + c), rnd((p, c), dt, 203 + c)
        o1, o2 = _rowdot(cuda, dt, a, b, p, c), _rowdot(cuda, dt, a, b, p, c)
        # inputs are exact in dt and the sum is fp32 for both dtypes
        close(o1[:p], (a * b).sum(1), torch.float32)
        assert torch.equal(o1, o2)


@pytest.mark.parametrize("dt", DTS)
def test_rowdot_seg(cuda, dt):
    """Laid out as coatt_flash_bwd uses it: row n * hw + j -> out[n * hwp + j]; the padding
    entries [hw, hwp) of every segment are left alone."""
    n, hw, hwp, c = 3, 13, 32, 256
    p = n * hw
    a, b = ints((p, c), 210), ints((p, c), 211)
    out = _rowdot(cuda, dt, a, b, p, c, hw, hwp).view(n, hwp)
    assert torch.equal(out[:, :hw].cpu(), (a * b).sum(1).float().view(n, hw))
    assert bool((out[:, hw:] == SENT).all())
    a, b = rnd((p, c), dt, 212), rnd((p, c), dt, 213)
    o1 = _rowdot(cuda, dt, a, b, p, c, hw, hwp).view(n, hwp)
    o2 = _rowdot(cuda, dt, a, b, p, c, hw, hwp).view(n, hwp)
    close(o1[:, :hw], (a * b).sum(1).view(n, hw), torch.float32)
    assert torch.equal(o1, o2) and bool((o1[:, hw:] == SENT).all())


# ---- cn_cast2d -------------------------------------------------------------------------------
@pytest.mark.parametrize("di", DTS)
@pytest.mark.parametrize("do", DTS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_cast2d(cuda, di, do, accumulate):
    def check(src, dst, dbuf, c):
        d0 = dst.clone()
        ops.cast_copy(src, dst, accumulate=accumulate)
        torch.cuda.synchronize()
        want = (src.float() + d0.float()).to(do) if accumulate else src.to(do)
        assert torch.equal(dst, want)
        if dbuf is not None:
            assert outside_unchanged(dbuf, c, do)
    # both sides channel slices
    p, c = 37, 50
    src = sliced(rnd((p, c), di, 220), di, cuda, fill=1000.0)[1]
    dbuf, dst = sliced(rnd((p, c), do, 221), do, cuda)
    check(src, dst, dbuf, c)
    # one column (the flat gradient bucket viewed as [n, 1])
    n = 1031
    check(rnd((n,), di, 222).to(di).to(cuda).view(-1, 1), rnd((n,), do, 223).to(do).to(cuda).view(-1, 1),
          None, 1)
    # more elements than the capped grid has threads
    p, c = 1025, 1024
    assert p * c > 4096 * 256
    check(rnd((p, c), di, 224).to(di).to(cuda), rnd((p, c), do, 225).to(do).to(cuda), None, c)


# ---- cn_weight_prep --------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", [(64, 3, 7, 8, False), (70, 36, 1, None, True), (96, 64, 3, None, True)])
def test_weight_prep(cuda, dt, case):
    cout, cin, k, cin_pad, need_t = case
    w = rnd((cout, cin, k, k), torch.float32, 230).float()
    wg = w.to(cuda).contiguous(memory_format=torch.channels_last)
    wf, wt = ops.WeightCache().get(wg, dt, cin_pad=cin_pad, need_t=need_t)
    torch.cuda.synchronize()
    cp = cin_pad or cin
    want = torch.zeros((cout, k, k, cp), dtype=torch.float32)
    want[..., :cin] = w.permute(0, 2, 3, 1)
    assert wf.dtype == dt and torch.equal(wf.cpu(), want.reshape(cout, k * k * cp).to(dt))
    assert bool((wf.view(cout, k * k, cp)[:, :, cin:] == 0).all())
    if need_t:
        assert wt.dtype == dt
        assert torch.equal(wt.cpu(), w.permute(1, 2, 3, 0).reshape(cin, k * k * cout).to(dt))
    else:
        assert wt is None


# ---- cn_splitk_reduce ------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [1, 2, 7, 16, 33])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("pad", [0, 8])
def test_splitk_reduce(cuda, nsplit, accumulate, pad):
    """out[i] (+)= sum over the splits of ws[s * slab + i], i < n; with slab > n the tail of every
    slab holds values that would wreck the sums if the slab stride and n were confused."""
    n = 4 * 131
    slab = n + pad

    def run(w, o0):
        wg = torch.full((nsplit, slab), 1000.0, dtype=torch.float32, device=cuda)
        wg[:, :n].copy_(w)
        out = torch.full((n + 4,), SENT, dtype=torch.float32, device=cuda)
        out[:n].copy_(o0)
        nv.call("cn_splitk_reduce", wg.data_ptr(), nsplit, slab, n, out.data_ptr(), accumulate, nv.stream())
        torch.cuda.synchronize()
        assert bool((out[n:] == SENT).all())
        return out[:n]

    wi, o0 = ints((nsplit, n), 240 + nsplit), ints((n,), 241)
    assert torch.equal(run(wi, o0).cpu(), (wi.sum(0) + accumulate * o0).float())
    wr, o0 = rnd((nsplit, n), torch.float32, 242 + nsplit), rnd((n,), torch.float32, 243)
    o1, o2 = run(wr, o0), run(wr, o0)
    close(o1, wr.sum(0) + accumulate * o0, torch.float32)
    assert torch.equal(o1, o2)


# ---- argument checks -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_channel_counts_off_the_vector_width_are_refused(cuda, dt):
    """These kernels walk C / V whole 16-byte chunks: a C that is no multiple of V would leave the
    last channels uncomputed, so the entry points refuse it before launching anything.  (The
    buffers are sized for the next multiple of V.)"""
    v = vec(dt)
    c, cw, p = 2 * v + 1, 3 * v, 8
    code = nv.dtype_code(dt)
    st = nv.stream()
    act = lambda: torch.full((p, cw), SENT, dtype=dt, device=cuda)
    f32 = lambda n: torch.full((n,), SENT, dtype=torch.float32, device=cuda)
    a, b, o, o2 = act(), act(), act(), act()
    w, bias, row, row2 = f32(cw), f32(1), f32(p), f32(p)
    ws = torch.empty((int(nv.query("cn_colpart_workspace_floats", p, cw)),), dtype=torch.float32, device=cuda)
    am = torch.full((p * cw,), 77, dtype=torch.uint8, device=cuda)
    calls = {
        "cn_rowdot_seg": (code, a.data_ptr(), cw, b.data_ptr(), cw, p, c, p, p, row.data_ptr(), st),
        "cn_rowdot": (code, a.data_ptr(), cw, b.data_ptr(), cw, p, c, row.data_ptr(), st),
        "cn_bcast_rows": (code, a.data_ptr(), 2, 4, c, 1.0, o.data_ptr(), cw, 0, st),
        "cn_gate_fwd": (code, a.data_ptr(), cw, p, c, w.data_ptr(), bias.data_ptr(), o.data_ptr(), cw,
                        row.data_ptr(), st),
        "cn_gate_bwd": (code, a.data_ptr(), cw, b.data_ptr(), cw, row2.data_ptr(), p, c, w.data_ptr(), 1,
                        o.data_ptr(), cw, o2.data_ptr(), row.data_ptr(), ws.data_ptr(), st),
        "cn_head_fwd": (code, a.data_ptr(), cw, b.data_ptr(), cw, p, c, 1, w.data_ptr(), bias.data_ptr(),
                        o.data_ptr(), cw, row.data_ptr(), st),
        "cn_head_bwd": (code, a.data_ptr(), cw, row2.data_ptr(), p, c, 1, w.data_ptr(), o.data_ptr(), cw,
                        o2.data_ptr(), row.data_ptr(), ws.data_ptr(), st),
        # 1 x 4 x 2 image -> 2 x 1 (k 3, s 2, pad 1), channel count c
        "cn_maxpool_fwd": (code, a.data_ptr(), 1, 4, 2, c, 2, 1, 3, 2, 1, o.data_ptr(), am.data_ptr(), st),
        "cn_maxpool_bwd": (code, a.data_ptr(), am.data_ptr(), 1, 4, 2, c, 2, 1, 3, 2, 1, o.data_ptr(), st),
    }
    for name, args in calls.items():
        with pytest.raises(nv.NativeError, match="alignment"):
            nv.call(name, *args)
    torch.cuda.synchronize()
    for t in (o, o2, row, a, b):
        assert bool((t == SENT).all())
    assert bool((am == 77).all())


# ---- fp8 quantisation (fp8.hip) --------------------------------------------------------------
def _dec_e4m3(u8):
    return u8.cpu().view(torch.float8_e4m3fn).double()


def _fp8_slice_case(cuda, dt, p, c):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((p, c), generator=g) * 3.0).to(dt)
    cat = torch.full((p, c + 24), 1000.0, dtype=dt, device=cuda)     # ld % 8 == 0 for both dtypes
    cat8 = torch.full((p, c + 16), 0x5A, dtype=torch.uint8, device=cuda)
    cat[:, :c].copy_(x)
    st = ops.fp8_state(cuda)
    y8 = ops.fp8_quant(cat[:, :c], st, ops.FP8_CURRENT, out=cat8[:, :c])
    torch.cuda.synchronize()
    assert y8.data_ptr() == cat8.data_ptr()
    assert bool((cat8[:, c:] == 0x5A).all())
    amax = x.double().abs().max().item()
    assert abs(st[0].item() - amax / 448) <= 1e-6 * amax
    ref = (x.double() * st[1].double().cpu()).clamp(-448, 448).to(torch.float8_e4m3fn)
    got = _dec_e4m3(cat8[:, :c].contiguous())
    diff = (got - ref.double()).abs()
    ulp = ref.double().abs().clamp_min(2 ** -6) * 2 ** -3   # one e4m3 mantissa step
    assert (diff <= ulp * 1.001).all()
    assert (diff == 0).double().mean().item() >= 0.999     # ties only may differ
    return cat, cat8, x, st


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("p", [1, 5, 260])
def test_fp8_quant_on_slices(cuda, dt, p):
    c = 72
    cat, cat8, x, st = _fp8_slice_case(cuda, dt, p, c)
    # amax-only mode: nothing but state[2] changes, no byte is written
    s0 = torch.tensor([0.5, 2.0, 0.0, 448.0], dtype=torch.float32, device=cuda)
    b0 = cat8.clone()
    ops.fp8_quant(cat[:, :c], s0, ops.FP8_AMAX, out=cat8[:, :c])
    torch.cuda.synchronize()
    assert s0.tolist() == [0.5, 2.0, x.float().abs().max().item(), 448.0]
    assert torch.equal(cat8, b0)
    # an all-zero tensor under current scaling keeps the previous scale
    cat[:, :c].zero_()
    s1 = torch.tensor([0.5, 2.0, 0.0, 448.0], dtype=torch.float32, device=cuda)
    ops.fp8_quant(cat[:, :c], s1, ops.FP8_CURRENT, out=cat8[:, :c])
    torch.cuda.synchronize()
    assert s1.tolist() == [0.5, 2.0, 0.0, 448.0]
    assert bool((cat8[:, :c] == 0).all()) and bool((cat8[:, c:] == 0x5A).all())


@pytest.mark.parametrize("dt", DTS)
def test_fp8_quant_row_block_cap(cuda, dt):
    """One chunk column, P > 64 * 1024: the row-block count is capped at 1024."""
    _fp8_slice_case(cuda, dt, 65600, 8)


def test_fp8_quant_multi_is_the_separate_launches(cuda):
    """cn_fp8_quant_multi (the table Fp8Weights.refresh_all builds): the bytes and the state of
    every record are bitwise those of one cn_fp8_quant_fmt(FP8_CURRENT) call on the same tensor
    from the same initial state."""
    g = torch.Generator().manual_seed(250)
    mk = lambda p, c, dt, ldx: (torch.randn((p, ldx), generator=g) * 2.0).to(dt).to(cuda)[:, :c]
    xs = [mk(300, 64, torch.float32, 64),       # more rows than the 128 row blocks
          mk(7, 2056, torch.float32, 2056),     # 257 chunks a row: more than one per thread
          mk(130, 72, torch.bfloat16, 96),      # bf16 source with ld > C
          torch.zeros((5, 16), dtype=torch.float32, device=cuda)]
    init = [0.7, 1.0 / 0.7, 0.0, 448.0]
    blob, outs, sts = b"", [], []
    for x in xs:
        p, c = x.shape
        y = torch.full((p, c), 0x5A, dtype=torch.uint8, device=cuda)
        st = torch.tensor(init, dtype=torch.float32, device=cuda)
        blob += fp8mod._REC.pack(x.data_ptr(), ops.ld(x), p, c, y.data_ptr(), c, st.data_ptr(),
                                 int(x.dtype == torch.bfloat16))
        outs.append(y)
        sts.append(st)
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(cuda)
    nv.call("cn_fp8_quant_multi", table.data_ptr(), len(xs), nv.stream())
    torch.cuda.synchronize()
    for x, y, st in zip(xs, outs, sts):
        st1 = torch.tensor(init, dtype=torch.float32, device=cuda)
        y1 = ops.fp8_quant(x, st1, ops.FP8_CURRENT)
        torch.cuda.synchronize()
        assert torch.equal(y, y1), tuple(x.shape)
        assert torch.equal(st.view(torch.int32), st1.view(torch.int32)), tuple(x.shape)
    assert sts[3].tolist() == torch.tensor(init, dtype=torch.float32).tolist()
    assert sts[0][0].item() != sts[3][0].item()
