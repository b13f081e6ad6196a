"""The input generators of tests/test_gpu_exact_gemm.py, checked without a GPU: for every case of
that file the inputs and the fp64 reference are built here and must meet the conditions the
bitwise comparison rests on -- the exactness bound (every partial sum below 2^24), an integral
reference (a multiple of the power-of-two scale where one applies), at least 10 % exact bf16 ties
wherever a bias or an old C offsets the outputs, |reference| <= 256 in the representable regime --
so a wrong generator cannot make the GPU tests vacuous."""
import torch

import test_gpu_exact_gemm as E


def test_cpu_cast_rounds_to_nearest_even():
    v = torch.tensor([257.0, 259.0, 261.0, 514.0, 518.0], dtype=torch.float64)
    assert E.rne_bf16(v).double().tolist() == [256.0, 260.0, 260.0, 512.0, 520.0]
    assert E.is_tie(v).all() and not E.is_tie(torch.tensor([256.0, 258.0, 513.0, 0.0])).any()


def test_generators():
    x = E.ints((4000,), -4, 4, 1)
    assert x.dtype == torch.float64 and set(x.tolist()) == set(range(-4, 5))
    assert torch.equal(x, E.ints((4000,), -4, 4, 1)) and not torch.equal(x, E.ints((4000,), -4, 4, 2))
    b = E.offset_bias(64, 3)
    assert ((b.abs() - 384).abs() <= 8).all() and (b[0::2] > 0).all() and (b[1::2] < 0).all()
    o = E.old_c((64, 64), 5)
    assert (o % 2 == 0).all() and (o.abs() >= 256).all() and (o.abs() <= 510).all()
    assert (o > 0).any() and (o < 0).any() and torch.equal(E.rne_bf16(o).double(), o)
    for fmt, vals in ((E.E4M3, 2 * E.ints((999,), -4, 4, 6)), (E.E4M3, 4 * E.ints((999,), -3, 3, 7)),
                      (E.E5M2, E.ints((999,), -4, 4, 8))):
        assert torch.equal(E.fp8_bytes(vals, fmt).view(fmt).double(), vals)
    nan = torch.tensor([E.FP8_NAN], dtype=torch.uint8)
    assert nan.view(E.E4M3).float().isnan().all() and nan.view(E.E5M2).float().isnan().all()


def test_every_case_meets_its_conditions():
    """Prints the tie share of every offset comparison (pytest -s shows the table)."""
    shares = []
    for label, out in E.all_problems():
        share = E.verify(out)
        if out.ties:
            shares.append((share, label))
    assert len(shares) >= 40
    for share, label in shares:
        print("ties %5.1f %%  %s" % (100 * share, label))
    print("minimum tie share %.1f %% (condition: >= %.0f %%)" % (100 * min(shares)[0], 100 * E.MIN_TIES))
    assert min(shares)[0] >= E.MIN_TIES
