"""Indexed flash co-attention forward (cn_coatt_fused_fwd_idx): operands are feature banks
[T*HW][ld] and each pair names its a-role and b-role frame through device int32 maps
(rgbd_segmentation_RAA.py:160-170 for the (target, reference) pairs of test.py:287-305).

The indexed call must be BITWISE cn_coatt_fused_fwd_ws on gathered stacked copies at the same
(P, HW, ndir) and workspace size -- the work plan is then the same and only the operand addresses
differ -- for the default 48-row kernel (variant 5) and the 4-wave kernel (variant 1).  Shapes:

    HW = 40    one partial row block, partial last key tile
    HW = 200   two row blocks (second partial), 7 key tiles; with 6 pairs the planner cuts items
               across workgroups: the partial-merge path
    HW = 3600  configs[3]'s map

Banks are strided views (ld > C) inside NaN-filled buffers and hold one unused frame of NaN, so a
read outside the named frames shows; the maps repeat an a-frame, hold a pair with ia == ib and are
not monotone; outputs sit in sentinel-filled buffers.
"""
import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

pytestmark = pytest.mark.gpu

C = 256
TOL = 1.5e-2          # of the output scale, as tests/test_gpu_coatt_fused.py
SENT = 123.0          # output sentinel (exact in bf16)
LDB, OFFB = 320, 64   # bank row stride and column offset of the view
LDZ, GUARD = 264, 3   # output row stride, guard rows before and after

# HW -> (frames T, unused frame, ia, ib)
CASES = {
    40: (4, 2, [3, 3, 0], [1, 3, 0]),
    200: (6, 4, [5, 5, 5, 0, 2, 1], [3, 5, 0, 0, 1, 2]),
    3600: (5, 1, [4, 4, 2, 0, 4], [0, 3, 2, 4, 2]),
}
_cache = {}


def bank_case(hw, cuda):
    """Banks, maps and gathered stacked copies of one shape (built once, never modified)."""
    if hw in _cache:
        return _cache[hw]
    t, unused, ia, ib = CASES[hw]
    assert unused not in ia and unused not in ib and max(ia + ib) < t
    g = torch.Generator().manual_seed(1000 + hw)
    banks = []
    for _ in range(3):   # vat, va, vb
        buf = torch.full((t * hw + 2, LDB), float("nan"), dtype=torch.bfloat16)
        x = (torch.randn((t * hw, C), generator=g) * 0.8).to(torch.bfloat16)
        x[unused * hw:(unused + 1) * hw] = float("nan")
        buf[1:1 + t * hw, OFFB:OFFB + C] = x
        buf = buf.to(cuda)
        view = buf[1:1 + t * hw, OFFB:OFFB + C]
        assert ops.ld(view) == LDB and view.data_ptr() % 16 == 0
        banks.append(view)
    rows = lambda idx: torch.cat([torch.arange(f * hw, (f + 1) * hw) for f in idx]).to(cuda)
    ra, rb = rows(ia), rows(ib)
    stacked = (banks[0][ra].contiguous(), banks[1][ra].contiguous(), banks[2][rb].contiguous())
    maps = (torch.tensor(ia, dtype=torch.int32, device=cuda), torch.tensor(ib, dtype=torch.int32, device=cuda))
    _cache[hw] = (banks, maps, stacked, len(ia))
    return _cache[hw]


def out_buf(p, hw, cuda):
    buf = torch.full((p * hw + 2 * GUARD, LDZ), SENT, dtype=torch.bfloat16, device=cuda)
    view = buf[GUARD:GUARD + p * hw, :C]
    assert view.data_ptr() % 16 == 0
    return buf, view


def sentinels_intact(buf, p, hw):
    s = torch.tensor(SENT, dtype=torch.bfloat16, device=buf.device)
    return bool((buf[:GUARD] == s).all() and (buf[GUARD + p * hw:] == s).all()
                and (buf[GUARD:GUARD + p * hw, C:] == s).all())


def launch(entry, ops3, maps, p, hw, which, cuda):
    """One forward through `entry` into fresh sentinel buffers; returns {name: (buffer, view)}."""
    vat, va, vb = ops3
    outs = {k: out_buf(p, hw, cuda) for k in ("za", "zb") if which in ("both", k)}
    za = outs["za"][1] if "za" in outs else None
    zb = outs["zb"][1] if "zb" in outs else None
    nws = int(nv.query("cn_coatt_fused_workspace_bytes", p, hw, len(outs)))
    ws = torch.empty((max(nws, 16) // 4,), dtype=torch.float32, device=cuda)
    args = [vat.data_ptr(), ops.ld(vat), va.data_ptr(), ops.ld(va), vb.data_ptr(), ops.ld(vb)]
    if entry == "cn_coatt_fused_fwd_idx":
        args += [nv.ptr(maps[0]), nv.ptr(maps[1])]
    args += [p, hw, C, nv.ptr(za), nv.ptr(zb), LDZ, ws.data_ptr(), nws, nv.stream()]
    nv.call(entry, *args)
    torch.cuda.synchronize()
    return outs


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture
def variant(request):
    lib = nv.load()
    old = lib.cn_coatt_force_variant(request.param)
    assert old != -1
    yield request.param
    lib.cn_coatt_force_variant(old)


@pytest.mark.parametrize("variant", [5, 1], indirect=True)
@pytest.mark.parametrize("which", ["za", "zb", "both"])
@pytest.mark.parametrize("hw", [40, 200, 3600])
def test_indexed_is_bitwise_the_stacked_call(cuda, hw, which, variant):
    banks, maps, stacked, p = bank_case(hw, cuda)
    ref = launch("cn_coatt_fused_fwd_ws", stacked, None, p, hw, which, cuda)
    got = launch("cn_coatt_fused_fwd_idx", banks, maps, p, hw, which, cuda)
    null = launch("cn_coatt_fused_fwd_idx", stacked, (None, None), p, hw, which, cuda)
    assert set(got) == set(ref) == ({"za", "zb"} if which == "both" else {which})
    for k in ref:
        assert sentinels_intact(ref[k][0], p, hw), k
        assert torch.isfinite(ref[k][1].float()).all(), k
        assert sentinels_intact(got[k][0], p, hw), (k, "indexed call wrote outside its rows")
        assert torch.equal(bits(got[k][0]), bits(ref[k][0])), \
            (k, (got[k][1].float() - ref[k][1].float()).abs().max().item())
        assert torch.equal(bits(null[k][0]), bits(ref[k][0])), (k, "NULL maps differ from the stacked entry")


@pytest.mark.parametrize("variant", [5, 1], indirect=True)
@pytest.mark.parametrize("shared", [False, True])
def test_indexed_vs_fp64(cuda, variant, shared):
    """Independent of the stacked entry: fp64 softmax of the indexed frames (HW = 200).  shared:
    vb is the va bank itself, as whole-sequence inference passes it."""
    hw = 200
    banks, maps, stacked, p = bank_case(hw, cuda)
    vat_s, va_s, vb_s = stacked
    if shared:
        banks = (banks[0], banks[1], banks[1])
        rb = torch.cat([torch.arange(f * hw, (f + 1) * hw) for f in CASES[hw][3]]).to(cuda)
        vb_s = banks[1][rb].contiguous()
    got = launch("cn_coatt_fused_fwd_idx", banks, maps, p, hw, "both", cuda)
    qa = vat_s.double().reshape(p, hw, C)
    a = va_s.double().reshape(p, hw, C)
    b = vb_s.double().reshape(p, hw, C)
    S = qa @ b.transpose(1, 2)
    ra = (torch.softmax(S, dim=2) @ b).reshape(p * hw, C)
    rb_ = (torch.softmax(S, dim=1).transpose(1, 2) @ a).reshape(p * hw, C)
    for k, ref in (("za", ra), ("zb", rb_)):
        z = got[k][1]
        assert torch.isfinite(z.float()).all(), k
        e = ((z.double() - ref).abs().max() / ref.abs().max()).item()
        print("indexed %s vs fp64 (variant %d, shared %s): %.3e of the output scale" % (k, variant, shared, e))
        assert e <= TOL, (k, e)


def test_ops_wrapper_and_shape_check(cuda):
    """ops.coatt_fused_idx (own workspace) gives the same bits; C != 256 is refused."""
    hw = 40
    banks, maps, stacked, p = bank_case(hw, cuda)
    ref = launch("cn_coatt_fused_fwd_idx", banks, maps, p, hw, "za", cuda)["za"][1]
    za = torch.empty((p * hw, C), dtype=torch.bfloat16, device=cuda)
    r = ops.coatt_fused_idx(banks[0], banks[1], banks[2], maps[0], maps[1], p, hw, za=za)
    torch.cuda.synchronize()
    assert r[1] is None and torch.equal(bits(za), bits(ref))
    with pytest.raises(ValueError):   # maps must be int32 on the GPU
        ops.coatt_fused_idx(banks[0], banks[1], banks[2], maps[0].long(), maps[1], p, hw, za=za)
    narrow = [b[:, :128] for b in banks]
    with pytest.raises(nv.NativeError):
        ops.coatt_fused_idx(narrow[0], narrow[1], narrow[2], maps[0], maps[1], p, hw,
                            za=torch.empty((p * hw, 128), dtype=torch.bfloat16, device=cuda))
