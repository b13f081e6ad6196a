"""MX-fp8 co-attention over a feature bank (cn_coatt_f8_bank_build, cn_coatt_f8_fwd_idx): every
frame's MX images are built once, and each pair names its query frame and its key / value frame
through device int32 maps (rgbd_segmentation_RAA.py:160-170 / :213-221 for the (target, reference)
pairs of test.py:287-305).

The indexed call must be BITWISE the za of cn_coatt_f8_fwd on gathered stacked copies (vat[ia],
va[ia], vb = va[ib]): an MX image is a function of its own frame's rows only, so the bank holds
the bytes the dense prepass writes, and only the operand addresses differ.  Shapes:

    HW = 40    one partial query block, one partial key tile (the nt == 1 path of the 3-stage ring)
    HW = 200   two query blocks (second partial), four key tiles, the last holding 8 keys
    HW = 3600  configs[3]'s map

Recipe of tests/test_gpu_coatt_idx.py: banks are strided views (ld 320, column offset 64) inside
NaN-filled buffers and hold one unused frame of NaN (its image is built -- ordinary data -- but
never read); the maps repeat an a-frame, hold a pair with ia == ib and are not monotone; outputs
sit in sentinel-filled buffers with guard rows; features are randn * 1.0 in bf16.

Independent of the dense entry: fp64 softmax on the kernel's own MX-dequantised operands (the
emulation of tests/test_gpu_coatt_f8.py), with that comparison's bounds.
"""
import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

pytestmark = pytest.mark.gpu

C = 256
SENT = 123.0          # output sentinel (exact in bf16)
LDB, OFFB = 320, 64   # bank row stride and column offset of the view
LDZ, GUARD = 264, 3   # output row stride, guard rows before and after
TAIL = 512            # sentinel bytes behind an image bank
TAILV = 0xA5

# HW -> (frames T, unused frame, ia, ib): the cases of tests/test_gpu_coatt_idx.py
CASES = {
    40: (4, 2, [3, 3, 0], [1, 3, 0]),
    200: (6, 4, [5, 5, 5, 0, 2, 1], [3, 5, 0, 0, 1, 2]),
    3600: (5, 1, [4, 4, 2, 0, 4], [0, 3, 2, 4, 2]),
    400: (3, None, [2, 0, 2], [1, 0, 2]),          # the fp64 comparison: T = 3, P = 3
}
_cache = {}


def frame_rows(idx, hw, dev):
    return torch.cat([torch.arange(f * hw, (f + 1) * hw) for f in idx]).to(dev)


def bank_case(hw, cuda, mod=0):
    """(vat, va) banks of modality `mod`, maps and gathered stacked copies (vat[ia], va[ia],
    va[ib]) of one shape; built once, never modified."""
    key = (hw, mod)
    if key in _cache:
        return _cache[key]
    t, unused, ia, ib = CASES[hw]
    assert unused not in ia and unused not in ib and max(ia + ib) < t
    g = torch.Generator().manual_seed(2000 + hw + 7 * mod)
    banks = []
    for _ in range(2):   # vat, va
        buf = torch.full((t * hw + 2, LDB), float("nan"), dtype=torch.bfloat16)
        x = (torch.randn((t * hw, C), generator=g) * 1.0).to(torch.bfloat16)
        if unused is not None:
            x[unused * hw:(unused + 1) * hw] = float("nan")
        buf[1:1 + t * hw, OFFB:OFFB + C] = x
        buf = buf.to(cuda)
        view = buf[1:1 + t * hw, OFFB:OFFB + C]
        assert ops.ld(view) == LDB and view.data_ptr() % 16 == 0
        banks.append(view)
    ra, rb = frame_rows(ia, hw, cuda), frame_rows(ib, hw, cuda)
    stacked = (banks[0][ra].contiguous(), banks[1][ra].contiguous(), banks[1][rb].contiguous())
    maps = (torch.tensor(ia, dtype=torch.int32, device=cuda), torch.tensor(ib, dtype=torch.int32, device=cuda))
    _cache[key] = (banks, maps, stacked, t, len(ia))
    return _cache[key]


def build_image(vat, va, t, hw, cuda):
    """cn_coatt_f8_bank_build into a buffer with a sentinel tail; returns (buffer, bytes)."""
    nb = int(nv.query("cn_coatt_f8_bank_bytes", t, hw))
    hwp, ntile = (hw + 127) // 128 * 128, (hw + 63) // 64
    assert nb == 2 * t * hwp * 264 + t * ntile * 16896      # rows + scales (Q, K), V^T tiles + scales
    img = torch.full((nb + TAIL,), TAILV, dtype=torch.uint8, device=cuda)
    assert img.data_ptr() % 256 == 0
    nv.call("cn_coatt_f8_bank_build", vat.data_ptr(), ops.ld(vat), va.data_ptr(), ops.ld(va), t, hw, C,
            img.data_ptr(), nb, nv.stream())
    torch.cuda.synchronize()
    assert (img[nb:] == TAILV).all(), "the image build wrote behind its buffer"
    return img, nb


def image_of(hw, cuda, mod=0, stacked=False):
    key = ("img", hw, mod, stacked)
    if key not in _cache:
        banks, _, st, t, p = bank_case(hw, cuda, mod)
        if stacked:   # a bank whose frame i is pair i's: vat[ia] and, as K / V, va[ib]
            _cache[key] = build_image(st[0], st[2], p, hw, cuda)[0]
        else:
            _cache[key] = build_image(banks[0], banks[1], t, hw, cuda)[0]
    return _cache[key]


def out_buf(p, hw, cuda):
    buf = torch.full((p * hw + 2 * GUARD, LDZ), SENT, dtype=torch.bfloat16, device=cuda)
    view = buf[GUARD:GUARD + p * hw, :C]
    assert view.data_ptr() % 16 == 0
    return buf, view


def sentinels_intact(buf, p, hw):
    s = torch.tensor(SENT, dtype=torch.bfloat16, device=buf.device)
    return bool((buf[:GUARD] == s).all() and (buf[GUARD + p * hw:] == s).all()
                and (buf[GUARD:GUARD + p * hw, C:] == s).all())


def bits(t):
    return t.contiguous().view(torch.int16)


def fwd_idx(imgs, t, maps, p, hw, cuda):
    """One cn_coatt_f8_fwd_idx over one or two image banks into fresh sentinel buffers."""
    outs = [out_buf(p, hw, cuda) for _ in imgs]
    img1 = imgs[1].data_ptr() if len(imgs) == 2 else None
    za1 = outs[1][1].data_ptr() if len(imgs) == 2 else None
    nv.call("cn_coatt_f8_fwd_idx", imgs[0].data_ptr(), img1, t, nv.ptr(maps[0]), nv.ptr(maps[1]), p, hw, C,
            outs[0][1].data_ptr(), za1, LDZ, nv.stream())
    torch.cuda.synchronize()
    return outs


def dense_za(stacked, p, hw, cuda):
    """za of cn_coatt_f8_fwd on the stacked copies (zb computed and dropped)."""
    vat, va, vb = stacked
    (abuf, za), (_, zb) = out_buf(p, hw, cuda), out_buf(p, hw, cuda)
    nws = int(nv.query("cn_coatt_f8_workspace_bytes", p, hw))
    ws = torch.empty((nws,), dtype=torch.uint8, device=cuda)
    nv.call("cn_coatt_f8_fwd", vat.data_ptr(), ops.ld(vat), va.data_ptr(), ops.ld(va), vb.data_ptr(),
            ops.ld(vb), p, hw, C, za.data_ptr(), zb.data_ptr(), LDZ, None, None, ws.data_ptr(), nws,
            nv.stream())
    torch.cuda.synchronize()
    return abuf, za


@pytest.mark.parametrize("hw", [40, 200, 3600])
def test_indexed_is_bitwise_the_dense_kernel_on_gathered_stacks(cuda, hw):
    banks, maps, stacked, t, p = bank_case(hw, cuda)
    ref_buf, ref = dense_za(stacked, p, hw, cuda)
    assert sentinels_intact(ref_buf, p, hw) and torch.isfinite(ref.float()).all()
    (got_buf, got), = fwd_idx([image_of(hw, cuda)], t, maps, p, hw, cuda)
    assert sentinels_intact(got_buf, p, hw), "indexed call wrote outside its rows"
    assert torch.isfinite(got.float()).all(), "the unused NaN frame was read"
    assert torch.equal(bits(got_buf), bits(ref_buf)), (got.float() - ref.float()).abs().max().item()
    # NULL maps: a bank of the gathered stacks, T = P
    (null_buf, _), = fwd_idx([image_of(hw, cuda, stacked=True)], p, (None, None), p, hw, cuda)
    assert torch.equal(bits(null_buf), bits(ref_buf)), "NULL maps differ from the dense entry"


def test_two_modalities_in_one_launch_equal_two_launches(cuda):
    hw = 200
    _, maps, _, t, p = bank_case(hw, cuda, 0)
    assert bank_case(hw, cuda, 1)[3:] == (t, p)
    i0, i1 = image_of(hw, cuda, 0), image_of(hw, cuda, 1)
    both = fwd_idx([i0, i1], t, maps, p, hw, cuda)
    one = [fwd_idx([i], t, maps, p, hw, cuda)[0] for i in (i0, i1)]
    assert not torch.equal(bits(one[0][0]), bits(one[1][0]))      # the modalities do differ
    for k in range(2):
        assert sentinels_intact(both[k][0], p, hw), k
        assert torch.isfinite(both[k][1].float()).all(), k
        assert torch.equal(bits(both[k][0]), bits(one[k][0])), k


# ---- fp64 on the kernel's own MX-dequantised operands (emulation of tests/test_gpu_coatt_f8.py) ----
def _scale_of(amax):
    e = torch.ceil(torch.log2(amax / 448.0))
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-126, 127)
    return torch.exp2(e)


def mx_rows(x):
    """[R, 256] -> dequantised MX rows (one E8M0 scale per 32 channels)."""
    r = x.shape[0]
    xb = x.double().reshape(r, 8, 32)
    sc = _scale_of(xb.abs().amax(-1))[..., None]
    return ((xb / sc).to(torch.float8_e4m3fn).double() * sc).reshape(r, 256)


def mx_vt(v, n, hw):
    """V [n*hw, 256] -> dequantised with one E8M0 scale per (channel, 32 consecutive keys of a
    64-key tile): the k-blocks of the scaled MFMA's PV product."""
    out = v.double().reshape(n, hw, 256).clone()
    for k0 in range(0, hw, 32):
        blk = out[:, k0:k0 + 32, :]
        sc = _scale_of(blk.abs().amax(1, keepdim=True))
        out[:, k0:k0 + 32, :] = (blk / sc).to(torch.float8_e4m3fn).double() * sc
    return out.reshape(n * hw, 256)


def test_indexed_vs_fp64_on_own_operands(cuda):
    """HW = 400, T = 3, P = 3, unit features: relative L2 <= 3e-2 and max <= 8e-2 of the output
    scale, the bounds of test_coatt_f8_vs_fp64 for exactly this comparison (only the e4m3 rounding
    of P and fp32 accumulation remain; the dense kernel is recorded at 0.5-1.3e-2 L2 for this
    input recipe, and the indexed output is bitwise the dense kernel's)."""
    hw = 400
    banks, maps, stacked, t, p = bank_case(hw, cuda)
    (buf, za), = fwd_idx([image_of(hw, cuda)], t, maps, p, hw, cuda)
    assert sentinels_intact(buf, p, hw) and torch.isfinite(za.float()).all()
    vat_s, _, vb_s = stacked
    q = mx_rows(vat_s).reshape(p, hw, C)
    k = mx_rows(vb_s).reshape(p, hw, C)
    v = mx_vt(vb_s, p, hw).reshape(p, hw, C)
    ref = (torch.softmax(q @ k.transpose(1, 2), dim=2) @ v).reshape(p * hw, C)
    l2 = ((za.double() - ref).norm() / ref.norm()).item()
    mx = ((za.double() - ref).abs().max() / ref.abs().max()).item()
    print("indexed fp8 za vs own-operand fp64 (hw 400, 3 pairs): L2 %.3e, max %.3e of the output scale" % (l2, mx))
    assert l2 <= 3e-2 and mx <= 8e-2, (l2, mx)


def test_ops_wrappers_and_errors(cuda):
    hw = 40
    banks, maps, stacked, t, p = bank_case(hw, cuda)
    raw = image_of(hw, cuda)
    nb = raw.numel() - TAIL
    img = ops.coatt_f8_bank(banks[0], banks[1], t, hw)
    torch.cuda.synchronize()
    assert img.dtype == torch.uint8 and img.numel() == nb and torch.equal(img, raw[:nb])
    ref = fwd_idx([raw], t, maps, p, hw, cuda)[0][1]
    za = torch.empty((p * hw, C), dtype=torch.bfloat16, device=cuda)
    r = ops.coatt_f8_idx(img, None, t, maps[0], maps[1], p, hw, za)
    torch.cuda.synchronize()
    assert r[0] is za and r[1] is None and torch.equal(bits(za), bits(ref))
    za2 = torch.empty_like(za)
    ops.coatt_f8_idx(img, img, t, maps[0], maps[1], p, hw, za, za2)
    torch.cuda.synchronize()
    assert torch.equal(bits(za), bits(ref)) and torch.equal(bits(za2), bits(ref))
    with pytest.raises(ValueError):   # maps must be int32 ...
        ops.coatt_f8_idx(img, None, t, maps[0].long(), maps[1], p, hw, za)
    with pytest.raises(ValueError):   # ... on the GPU
        ops.coatt_f8_idx(img, None, t, maps[0], maps[1].cpu(), p, hw, za)
    with pytest.raises(ValueError):   # the second modality is an image and an output, or neither
        ops.coatt_f8_idx(img, img, t, maps[0], maps[1], p, hw, za)
    with pytest.raises(nv.NativeError):   # C = 128
        ops.coatt_f8_idx(img, None, t, maps[0], maps[1], p, hw,
                         torch.empty((p * hw, 128), dtype=torch.bfloat16, device=cuda))
    with pytest.raises(nv.NativeError):
        ops.coatt_f8_bank(banks[0][:, :128], banks[1][:, :128], t, hw)
    with pytest.raises(ValueError):   # bf16 features only
        ops.coatt_f8_bank(banks[0].float(), banks[1].float(), t, hw)
    with pytest.raises(ValueError):   # fewer rows than t frames
        ops.coatt_f8_bank(banks[0], banks[1], t + 1, hw)
    with pytest.raises(ValueError):   # on the GPU
        ops.coatt_f8_bank(stacked[0].cpu(), stacked[1].cpu(), p, hw)
    # a too small image buffer is refused before anything is written
    small = torch.full((nb,), TAILV, dtype=torch.uint8, device=cuda)
    rc = nv.query("cn_coatt_f8_bank_build", banks[0].data_ptr(), LDB, banks[1].data_ptr(), LDB, t, hw, C,
                  small.data_ptr(), nb - 1, nv.stream())
    torch.cuda.synchronize()
    assert rc != 0 and (small == TAILV).all()
    # NULL maps name frame p: more pairs than frames is refused
    rc = nv.query("cn_coatt_f8_fwd_idx", img.data_ptr(), None, t, None, None, t + 1, hw, C, za.data_ptr(),
                  None, C, nv.stream())
    assert rc != 0
