"""CPU-side checks of the k-NN evaluation: the float64 references of knn_ref.py on hand-made cases (ties, a bank smaller than k, fewer than
five classes, labels outside the class range), the command line of main_knn.py and its refusals.  No kernel is launched."""
import math

import pytest
import torch

import knn_ref as R

INF = float("inf")


def test_select_ref_ties_go_to_the_lower_index():
    sim = torch.tensor([[0.5, 0.75, 0.5, 0.75, 0.125, 0.5],
                        [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    val, idx = R.select_ref(sim, 4)
    assert idx.dtype == torch.int32 and val.dtype == sim.dtype
    assert idx.tolist() == [[1, 3, 0, 2], [0, 1, 2, 3]]
    assert val.tolist() == [[0.75, 0.75, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0]]
    # chunked merging gives the same lists: select over the concatenation of per-chunk winners, with the winners' global indices
    a_val, a_idx = R.select_ref(sim[:, :3], 4)
    b_val, b_idx = R.select_ref(sim[:, 3:], 4)
    cat_val = torch.cat([a_val, b_val], 1)
    cat_idx = torch.cat([a_idx, torch.where(b_idx >= 0, b_idx + 3, b_idx)], 1)
    key = torch.argsort(cat_idx.masked_fill(cat_idx < 0, 1 << 30), dim=1, stable=True)   # back to index order, so the stable sort breaks ties by index
    m_val, pos = R.select_ref(torch.gather(cat_val, 1, key), 4)
    assert torch.equal(m_val, val) and torch.equal(torch.gather(torch.gather(cat_idx, 1, key), 1, pos.long()), idx)


def test_select_ref_bank_smaller_than_k():
    sim = torch.tensor([[0.25, -1.0, 0.75]])
    val, idx = R.select_ref(sim, 5)
    assert idx.tolist() == [[2, 0, 1, -1, -1]]
    assert val.tolist() == [[0.75, 0.25, -1.0, -INF, -INF]]


def test_vote_ref_weights_unused_slots_and_out_of_range_labels():
    T = 0.5
    val = torch.tensor([[1.0, 0.5, 0.5, 0.0, -INF]])
    idx = torch.tensor([[4, 0, 1, 2, -1]], dtype=torch.int32)
    bank_labels = torch.tensor([2, 0, 7, 9, 2])   # bank rows 2 and 3 carry labels outside [0, 3)
    votes, top5 = R.vote_ref(val, idx, bank_labels, 3, T)
    assert votes.dtype == torch.float64
    want = [math.exp(0.5 / T), 0.0, math.exp(1.0 / T) + math.exp(0.5 / T)]
    assert votes[0].tolist() == pytest.approx(want, rel=1e-15)
    assert top5.tolist() == [[2, 0, 1, -1, -1]]          # K < 5: the tail is -1; class 1 got no vote and still ranks
    assert R.hits_ref(top5, torch.tensor([2]), 3) == (1.0, 1.0)
    assert R.hits_ref(top5, torch.tensor([1]), 3) == (0.0, 1.0)
    assert R.hits_ref(top5, torch.tensor([-1]), 3) == (0.0, 0.0)   # must not match the -1 tail


def test_vote_ref_ties_go_to_the_lower_class():
    val = torch.tensor([[0.5, 0.5, 0.25]])
    idx = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    votes, top5 = R.vote_ref(val, idx, torch.tensor([5, 3, 6]), 8, 0.07)
    assert votes[0, 5] == votes[0, 3] > votes[0, 6] > 0
    assert top5.tolist() == [[3, 5, 6, 0, 1]]
    assert R.ranks_separated(votes) and float(R.top1_margin(votes)[0]) == 0.0
    assert not R.ranks_separated(torch.tensor([[1.0, 1.0 + 1e-6, 0.0]], dtype=torch.float64))


def test_knn_ref_pipeline_on_a_hand_made_bank():
    bank = torch.tensor([[2.0, 0.0], [0.0, 3.0], [1.0, 1.0], [0.0, 0.0]])     # row 3 is all zero: similarity 0 to everything
    queries = torch.tensor([[5.0, 0.0], [1.0, 1.0]])
    out = R.knn_ref(bank, queries, torch.tensor([0, 1, 1, 0]), K=2, k=3, T=0.5)
    r = math.sqrt(0.5)
    assert torch.allclose(out["sim"], torch.tensor([[1.0, 0.0, r, 0.0], [r, r, 1.0, 0.0]], dtype=torch.float64), atol=1e-15)
    assert out["idx"][0].tolist() == [0, 2, 1]            # the tie at 0 goes to bank row 1 before row 3
    assert out["idx"][1, 0].item() == 2
    assert out["top5"][:, 0].tolist() == [0, 1]


def test_cli_defaults_and_flags():
    import main_knn
    import main_linprobe
    import models_vit
    p = main_knn.get_args_parser()
    a = p.parse_args([])
    probe = main_linprobe.get_args_parser().parse_args([])
    for name in ("model", "finetune", "transform_checkpoint_keys", "global_pool", "input_size", "batch_size", "nb_classes", "train_path", "test_path",
                 "dataset_type", "num_workers", "device", "seed", "output_dir", "output_dir_base"):
        assert getattr(a, name) == getattr(probe, name), name
    assert a.model in models_vit.__dict__
    assert (a.knn_k, a.knn_t, a.knn_scales, a.bank_max, a.knn_dtype) == (20, 0.07, [1.0, 0.5, 0.25, 0.125], None, "bf16")
    b = p.parse_args(["--knn_scales", "1.0", "0.5", "--bank_max", "100", "--knn_dtype", "fp32", "--global_pool", "--knn_k", "5", "--knn_t", "0.1"])
    assert (b.knn_scales, b.bank_max, b.knn_dtype, b.global_pool, b.knn_k, b.knn_t) == ([1.0, 0.5], 100, "fp32", True, 5, 0.1)
    assert p.parse_args(["--global_pool", "--cls_token"]).global_pool is False
    with pytest.raises(SystemExit):
        p.parse_args(["--knn_dtype", "fp16"])
    assert [main_knn.scaled_size(s, 224) for s in a.knn_scales] == [224, 112, 56, 28]
    assert main_knn.scaled_size(0.3, 64) == 19
    with pytest.raises(ValueError, match="scale"):
        main_knn.scaled_size(1.5, 224)


def test_bank_subset_is_seeded_sorted_and_bounded():
    import main_knn
    assert main_knn.bank_subset(10, None, 0) is None and main_knn.bank_subset(10, 10, 0) is None and main_knn.bank_subset(10, 11, 0) is None
    s = main_knn.bank_subset(100, 7, 3)
    assert s.shape == (7,) and len(set(s.tolist())) == 7 and s.tolist() == sorted(s.tolist()) and 0 <= int(s.min()) and int(s.max()) < 100
    assert torch.equal(s, main_knn.bank_subset(100, 7, 3)) and not torch.equal(s, main_knn.bank_subset(100, 7, 4))
    with pytest.raises(ValueError, match="bank_max"):
        main_knn.bank_subset(10, 0, 0)


def test_refusals(monkeypatch, tmp_path):
    import main_knn
    from csmae_hip.knn import KnnIndex
    parse = main_knn.get_args_parser().parse_args
    with pytest.raises(NotImplementedError, match="sentinel"):
        main_knn.main(parse(["--dataset_type", "sentinel", "--output_dir", str(tmp_path)]))
    with pytest.raises(ValueError, match="knn_k"):
        main_knn.main(parse(["--dataset_type", "synthetic", "--knn_k", "65", "--output_dir", str(tmp_path)]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KnnIndex(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), 2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        main_knn.main(parse(["--dataset_type", "synthetic", "--output_dir", str(tmp_path)]))
