"""GPU tests of the k-NN evaluation (csrc/knn.hip, csmae_hip/knn.py, main_knn.py) against the float64 references of knn_ref.py, in guarded buffers:
l2_normalize, knn_select (bit-exact lists in any chunking), knn_vote, KnnIndex end to end in fp32 and bf16, and the driver on the micro ViT."""
import json

import pytest
import torch

import knn_ref as R
from finetune_ref import VAL, assert_close, guarded, guards_intact, write_pretrain_checkpoint

pytestmark = pytest.mark.gpu
INF = float("inf")
IDX_GUARD = -7777   # an int32 buffer cannot hold NaN: its guard rows hold this


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded_idx(rows, cols):
    big = torch.full((rows + 2, cols), IDX_GUARD, device="cuda", dtype=torch.int32)
    return big, big[1:rows + 1]


def idx_guards_intact(big):
    return bool((big[0] == IDX_GUARD).all()) and bool((big[-1] == IDX_GUARD).all())


# ------------------------------------------------------------------------------------------------ l2_normalize
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_l2_normalize(ops, dtype):
    rows, D, ld = 5, 130, 137
    big = torch.full((rows, ld), float("nan"))
    big[:, :D] = torch.randn(rows, D, generator=gen(1)) * torch.tensor([1.0, 1e-3, 50.0, 1.0, 7.0])[:, None]
    big[3, :D] = 0.0                                          # an all-zero row stays zero (0 / eps)
    src = big.cuda()[:, :D]
    ref = R.normalize_ref(big[:, :D])
    assert bool((ref[3] == 0).all())
    gbuf, out = guarded(rows, D, dtype)
    ops.l2_normalize(src, out)
    torch.cuda.synchronize()
    assert guards_intact(gbuf)
    if dtype == torch.float32:
        assert_close(out, ref, *VAL, what="l2_normalize fp32")
    else:
        err = (out.double().cpu() - ref).abs()
        print(f"l2_normalize bf16: worst err / |ref| {float((err / ref.abs().clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= 2.0 ** -8 * ref.abs()).all())   # one bf16 rounding of the fp64 value
    assert bool((out[3] == 0).all())


# ------------------------------------------------------------------------------------------------ knn_select
def run_select(ops, sim, k, chunks):
    """Merge `sim` [Q, B] (CPU fp32) tile by tile (`chunks`: column counts) into fresh guarded lists -> (val, idx) on the CPU.  Every tile has
    ld = Bc + 3 with +inf in the padding columns: a kernel that reads them lists them."""
    Q, B = sim.shape
    assert sum(chunks) == B
    vbig, val = guarded(Q, k)
    ibig, idx = guarded_idx(Q, k)
    val.fill_(-INF)
    idx.fill_(-1)
    b0 = 0
    for Bc in chunks:
        tile = torch.full((Q, Bc + 3), INF)
        tile[:, :Bc] = sim[:, b0:b0 + Bc]
        ops.knn_select(tile.cuda(), val, idx, base=b0, Bc=Bc)
        b0 += Bc
    torch.cuda.synchronize()
    assert guards_intact(vbig) and idx_guards_intact(ibig)
    return val.cpu(), idx.cpu()


def check_select(ops, sim, k, chunkings):
    rv, ri = R.select_ref(sim, k)
    for chunks in chunkings:
        val, idx = run_select(ops, sim, k, chunks)
        assert torch.equal(idx, ri), (chunks, idx, ri)
        assert torch.equal(val.view(torch.int32), rv.view(torch.int32)), chunks   # bit for bit (-inf included)
    return rv, ri


@pytest.mark.parametrize("Q,B,k", [(3, 200, 20), (2, 64, 64), (4, 37, 1), (2, 10, 20)])
def test_knn_select_exact(ops, Q, B, k):
    sim = torch.randn(Q, B, generator=gen(Q * 1000 + B + k))
    rv, ri = check_select(ops, sim, k, [[B]])
    if B < k:   # a bank smaller than k: the tail is (-inf, -1)
        assert bool((ri[:, B:] == -1).all()) and bool((rv[:, B:] == -INF).all())


def test_knn_select_ties_single_tile_and_chunked(ops):
    Q, B, k = 3, 1000, 20
    levels = torch.tensor([-0.5, -0.25, 0.0, 0.125, 0.25, 0.5, 0.75, 1.0])
    sim = levels[torch.randint(0, 8, (Q, B), generator=gen(5))]          # eight distinct values: nearly everything ties
    check_select(ops, sim, k, [[B], [333, 333, 334]])


def test_knn_select_aligned_rows_and_reversed_tiles(ops):
    """ld % 4 == 0 takes the float4 path (whole vectors, the scalar tail, more than one wave step); tiles merged last-to-first give the same lists."""
    Q, B, k = 5, 2345, 20
    sim = torch.randn(Q, B, generator=gen(6))
    sim[1] = sim[1].round()                                                   # many ties
    rv, ri = R.select_ref(sim, k)
    vbig, val = guarded(Q, k)
    ibig, idx = guarded_idx(Q, k)
    val.fill_(-INF)
    idx.fill_(-1)
    for b0, b1 in ((1200, 2345), (0, 1200)):
        Bc = b1 - b0
        ld = (Bc + 3) // 4 * 4 + 4
        tile = torch.full((Q, ld), INF)
        tile[:, :Bc] = sim[:, b0:b1]
        tile = tile.cuda()
        assert tile.data_ptr() % 16 == 0
        ops.knn_select(tile, val, idx, base=b0, Bc=Bc)
    torch.cuda.synchronize()
    assert guards_intact(vbig) and idx_guards_intact(ibig)
    assert torch.equal(idx.cpu(), ri) and torch.equal(val.cpu().view(torch.int32), rv.view(torch.int32))


def test_knn_select_ascending_and_descending_rows(ops):
    B, k = 300, 20
    up = torch.arange(B, dtype=torch.float32) / B                            # every element is an insertion
    sim = torch.stack([up, up.flip(0)])                                      # ... and behind the first k, none is
    check_select(ops, sim, k, [[B], [100, 200]])


@pytest.mark.parametrize("k", [0, 65])
def test_knn_select_refuses_k_outside_1_64(ops, k):
    import csmae_hip
    sim = torch.zeros(2, 8, device="cuda")
    val = torch.full((2, max(k, 1)), 3.0, device="cuda")
    idx = torch.full((2, max(k, 1)), 3, device="cuda", dtype=torch.int32)
    rc = csmae_hip.load().csmae_knn_select(2, 8, k, sim.data_ptr(), 8, 0, val.data_ptr(), idx.data_ptr(), ops.stream())
    assert rc == -1 and b"k = " in csmae_hip.load().csmae_last_error()
    if k:
        with pytest.raises(csmae_hip.CsmaeError, match="must lie in"):
            ops.knn_select(sim, val, idx)
    torch.cuda.synchronize()
    assert bool((val == 3.0).all()) and bool((idx == 3).all())              # nothing was launched


# ------------------------------------------------------------------------------------------------ knn_vote
def vote_case(Q, k, K, nbank, seed):
    g = gen(seed)
    val = torch.sort(torch.rand(Q, k, generator=g) * 1.2 - 0.2, dim=1, descending=True).values
    idx = torch.randint(0, nbank, (Q, k), generator=g).to(torch.int32)
    for q in range(Q):                                                       # lists with unused slots at the end, one of them nearly empty
        n = k - (q % 3) * 4 if q else 2
        val[q, n:], idx[q, n:] = -INF, -1
    bank_labels = torch.randint(0, K, (nbank,), generator=g)
    bank_labels[::11] = K + 2                                                # labels outside [0, K) vote for nothing
    bank_labels[5::13] = -1
    qlabels = torch.randint(0, K, (Q,), generator=g)
    qlabels[-1] = K                                                          # ... and a query label outside scores nothing
    return val, idx, bank_labels, qlabels


@pytest.mark.parametrize("Q,k,K,seed", [(6, 20, 7, 0), (6, 20, 3, 1)])
def test_knn_vote(ops, Q, k, K, seed):
    T = 0.07
    val, idx, bank_labels, qlabels = vote_case(Q, k, K, 50, seed)
    if K == 3:   # an exact tie from identical inputs: query 0's two neighbours carry the same similarity and labels 2 and 1
        val[0, :2] = 0.5
        bank_labels[int(idx[0, 0])], bank_labels[int(idx[0, 1])] = 2, 1
        assert int(idx[0, 0]) != int(idx[0, 1])
    rvotes, rtop5 = R.vote_ref(val, idx, bank_labels, K, T)
    assert R.ranks_separated(rvotes, 1e-3), "pick another seed: two ranked votes of the reference are closer than 1e-3 relative"
    assert bool((rvotes.sum(1) > 0).all())
    h1, h5 = R.hits_ref(rtop5, qlabels, K)
    dval, didx, dlab, dq = val.cuda(), idx.cuda(), bank_labels.cuda(), qlabels.cuda()
    vbig, votes = guarded(Q, K)
    tbig, top5 = guarded_idx(Q, 5)
    counts = torch.tensor([10.0, 20.0], device="cuda")
    ops.knn_vote(dval, didx, dlab, K, T, top5, votes=votes, counts=counts, query_labels=dq, accumulate_counts=False)
    torch.cuda.synchronize()
    assert guards_intact(vbig) and idx_guards_intact(tbig)
    assert_close(votes, rvotes, *VAL, what=f"knn_vote K={K}")
    assert torch.equal(top5.cpu(), rtop5), (top5.cpu(), rtop5)
    if K == 3:
        assert rtop5[0].tolist() == [1, 2, 0, -1, -1]                         # the tie went to the lower class, the tail is -1
    assert counts.tolist() == [h1, h5]
    ops.knn_vote(dval, didx, dlab, K, T, top5, counts=counts, query_labels=dq, accumulate_counts=True)   # (votes may be absent)
    assert counts.tolist() == [2 * h1, 2 * h5]
    assert torch.equal(top5.cpu(), rtop5)
    ops.knn_vote(dval, didx, dlab, K, T, top5, votes=votes, counts=counts, query_labels=None)            # no labels: counts stay
    assert counts.tolist() == [2 * h1, 2 * h5]


def test_knn_vote_many_classes(ops):
    """K = 1024: a lane walks 16 classes and the arg-max crosses lanes."""
    Q, k, K, T = 3, 20, 1024, 0.07
    g = gen(3)
    val = torch.linspace(1.0, 0.05, k).repeat(Q, 1) - 0.01 * torch.arange(Q)[:, None]   # distinct weights, well apart
    idx = torch.stack([torch.randperm(400, generator=g)[:k] for _ in range(Q)]).to(torch.int32)
    bank_labels = torch.randperm(K, generator=g)[:400]                       # every neighbour votes for a class of its own
    rvotes, rtop5 = R.vote_ref(val, idx, bank_labels, K, T)
    assert R.ranks_separated(rvotes, 1e-3)
    vbig, votes = guarded(Q, K)
    tbig, top5 = guarded_idx(Q, 5)
    ops.knn_vote(val.cuda(), idx.cuda(), bank_labels.cuda(), K, T, top5, votes=votes)
    torch.cuda.synchronize()
    assert guards_intact(vbig) and idx_guards_intact(tbig)
    assert_close(votes, rvotes, *VAL, what="knn_vote K=1024")
    assert torch.equal(top5.cpu(), rtop5)


# ------------------------------------------------------------------------------------------------ KnnIndex end to end
K_E2E, NOISE = 5, 1.5


@pytest.fixture(scope="module")
def e2e():
    g = gen(11)
    protos = torch.randn(K_E2E, 128, generator=g)
    bank_labels = torch.randint(0, K_E2E, (300,), generator=g)
    qlabels = torch.randint(0, K_E2E, (40,), generator=g)
    bank = protos[bank_labels] + NOISE * torch.randn(300, 128, generator=g)
    queries = protos[qlabels] + NOISE * torch.randn(40, 128, generator=g)
    ref = R.knn_ref(bank, queries, bank_labels, K_E2E, k=20, T=0.07)
    return dict(bank=bank, queries=queries, bank_labels=bank_labels, qlabels=qlabels, ref=ref)


@pytest.mark.parametrize("dtype,margin", [(torch.float32, 1e-3), (torch.bfloat16, 1e-2)])
def test_knn_index_end_to_end(ops, e2e, dtype, margin):
    from csmae_hip.knn import KnnIndex
    ref, k = e2e["ref"], 20
    stable = R.top1_margin(ref["votes"]) > margin
    assert int((~stable).sum()) <= 2, "choose another noise level or seed: too many queries sit on a vote margin"
    index = KnnIndex(e2e["bank"].cuda(), e2e["bank_labels"].cuda(), K_E2E, dtype=dtype)
    val, idx = index.search(e2e["queries"].cuda(), k, q_chunk=16, b_chunk=128)   # both loops run ragged: 16 + 16 + 8 queries, 128 + 128 + 44 rows
    val, idx = val.cpu().clone(), idx.cpu().clone()
    rval = ref["val"]
    if dtype == torch.float32:
        rtol, atol = VAL
    else:
        rtol, atol = 0.0, 3 * 2.0 ** -8   # |sim| <= 1 and both operands are rounded to bf16 once
    assert_close(val, rval, rtol, atol, what=f"KnnIndex {dtype} sorted top-k similarities")
    assert bool((val[:, :-1] >= val[:, 1:]).all())
    tol_kth = atol + rtol * rval[:, -1].abs()
    for q in range(idx.shape[0]):
        row = idx[q].long()
        assert len(set(row.tolist())) == k and int(row.min()) >= 0 and int(row.max()) < 300, (q, row)
        assert bool((ref["sim"][q, row] >= rval[q, -1] - tol_kth[q]).all()), q
    top5, votes = index.classify(e2e["queries"].cuda(), k=k, T=0.07, labels=e2e["qlabels"].cuda(), q_chunk=16, b_chunk=128)
    pred, rpred = top5[:, 0].cpu().long(), ref["top5"][:, 0].long()
    assert torch.equal(pred[stable], rpred[stable]), (pred, rpred)
    top1, top5_hits = index.counts.tolist()
    assert top1 == float((pred == e2e["qlabels"]).sum()) and top1 <= top5_hits <= 40
    assert votes.shape == (40, K_E2E)


# ------------------------------------------------------------------------------------------------ driver
def test_main_knn_on_the_micro_vit(ops, tmp_path):
    import main_knn
    ckpt = write_pretrain_checkpoint(tmp_path)
    out = tmp_path / "knn"
    flags = ["--dataset_type", "synthetic", "--model", "vit_base_patch16", "--embed_dim", "128", "--depth", "2", "--num_heads", "2", "--input_size", "64",
             "--batch_size", "8", "--synthetic_len", "4", "--nb_classes", "5", "--finetune", ckpt, "--transform_checkpoint_keys", "--bank_max", "20",
             "--knn_k", "5", "--knn_scales", "1.0", "0.5", "--output_dir", str(out)]
    results = main_knn.main(main_knn.get_args_parser().parse_args(flags))
    lines = [json.loads(ln) for ln in open(out / "log.txt")]
    assert len(lines) == 2 and lines == results
    for ln, scale in zip(lines, (1.0, 0.5)):
        assert set(ln) == set(main_knn.LOG_KEYS)
        assert ln["scale"] == scale and ln["knn_k"] == 5 and ln["knn_t"] == 0.07
        assert ln["bank_size"] == 20 and ln["n_queries"] == 8                # --bank_max of the 32 bank images; one validation batch
        assert 0.0 <= ln["top1"] <= ln["top5"] <= 100.0
        assert ln["extract_img_per_s"] > 0 and ln["search_s"] > 0
    # the synthetic queries are the bank's own batch: at full scale every query finds itself (when the subset kept its image) and its label
    assert lines[0]["top5"] >= lines[0]["top1"] > 0
