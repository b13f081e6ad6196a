"""Host side of whole-sequence inference: the pair plan (cosnet_amd.inference.plan_pairs) and the
loader's pixel-free reference plan (SBMRGBD.reference_plan, sbm_rgbd_loader.py:538-579)."""
import pytest
import torch

from cosnet_amd import sbm_rgbd as S
from cosnet_amd.inference import plan_pairs


def test_plan_pairs_is_target_major_in_reference_order():
    ia, ib = plan_pairs(6, [4, 0, 5], [[1, 2], [5, 3], [0, 4]])
    assert ia.dtype == ib.dtype == torch.int32 and not ia.is_cuda and not ib.is_cuda
    assert ia.tolist() == [4, 4, 0, 0, 5, 5]
    assert ib.tolist() == [1, 2, 5, 3, 0, 4]
    # CPU tensors as well as lists
    ia2, ib2 = plan_pairs(6, torch.tensor([4, 0, 5]), torch.tensor([[1, 2], [5, 3], [0, 4]]))
    assert torch.equal(ia, ia2) and torch.equal(ib, ib2)


def test_plan_pairs_accepts_self_references_and_repeats():
    # the reference's sampler draws the target itself and, across targets, the same frame again
    ia, ib = plan_pairs(3, [0, 1, 2], [[0, 0], [2, 1], [2, 2]])
    assert ia.tolist() == [0, 0, 1, 1, 2, 2] and ib.tolist() == [0, 0, 2, 1, 2, 2]


@pytest.mark.parametrize("targets,refs", [
    ([0, 3], [[1], [2]]),            # target outside the bank
    ([0, 1], [[1], [3]]),            # reference outside the bank
    ([0, 1], [[1], [-1]]),           # negative
    ([0, 1], [[1, 2], [0]]),         # ragged
    ([0, 1], [[], []]),              # N = 0
    ([0, 1], [[1]]),                 # one row of references for two targets
])
def test_plan_pairs_rejects(targets, refs):
    with pytest.raises(ValueError):
        plan_pairs(3, targets, refs)


def test_reference_plan_draws_what_getitem_loads(tmp_path, monkeypatch):
    """Two loaders with one seed: the first records the frames __getitem__ loads (pixels stubbed
    out), the second plans the same indices; (target, references...) must agree index by index,
    which also pins that reference_plan consumes the RNG exactly as __getitem__ does."""
    from test_sbm import _write_tree
    _write_tree(str(tmp_path), seqs=(("Shadows", "s1", 5), ("OutOfRange", "s2", 4), ("OutOfRange", "s3", 6)))
    mk = lambda: S.SBMRGBD(str(tmp_path), 3, (24, 32), for_training=False, batch_size=1,
                           subset_percentage=1.0, seed=77, device="cpu")
    a, b = mk(), mk()
    frames = a.sets["test"]["names_of_frames"]
    assert len(frames) == 15
    seen = []
    stub = torch.zeros((1, 2, 2))
    monkeypatch.setattr(a, "load_frame", lambda fi: seen.append(frames.index(fi)) or (stub, stub, stub[0]))
    for idx in range(len(a)):
        seen.clear()
        sample = a[idx]
        plan = b.reference_plan(idx)
        assert plan == seen, (idx, plan, seen)
        assert plan[0] == idx and len(plan) == 1 + 3
        r = b.sets["test"]["frame_range_of_sequences"][sample["seq_name"]]
        assert all(r["start"] <= f < r["end"] for f in plan)      # its own sequence
        assert len(set(plan[1:])) == 3                             # drawn without replacement
    assert a.rng.getstate() == b.rng.getstate()
    with pytest.raises(IndexError):
        b.reference_plan(15)
