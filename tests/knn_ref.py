"""Float64 CPU restatements of the k-NN evaluation (csrc/knn.hip, csmae_hip/knn.py) that test_knn_cpu.py checks on hand-made cases and
test_knn_gpu.py compares the kernels against."""
import torch


def select_ref(sim, k):
    """sim [Q, B] -> (val [Q, k] in sim's dtype, idx [Q, k] int32): a stable sort of every row by (descending value, ascending index) cut at k,
    padded with (-inf, -1) when B < k."""
    Q, B = sim.shape
    order = torch.argsort(sim, dim=1, descending=True, stable=True)[:, :k]
    val = torch.full((Q, k), float("-inf"), dtype=sim.dtype)
    idx = torch.full((Q, k), -1, dtype=torch.int32)
    n = min(k, B)
    val[:, :n] = torch.gather(sim, 1, order)
    idx[:, :n] = order.to(torch.int32)
    return val, idx


def vote_ref(val, idx, bank_labels, K, T):
    """DINO's weighted vote in float64 -> (votes [Q, K], top5 [Q, 5] int32).  Slots with idx < 0 and labels outside [0, K) vote for nothing;
    top5 ranks the classes by (descending vote, ascending class id), -1 behind the K-th when K < 5."""
    Q, k = val.shape
    votes = torch.zeros(Q, K, dtype=torch.float64)
    for q in range(Q):
        for j in range(k):
            i = int(idx[q, j])
            if i < 0:
                continue
            c = int(bank_labels[i])
            if 0 <= c < K:
                votes[q, c] += torch.exp(val[q, j].double() / T)
    top5 = torch.full((Q, 5), -1, dtype=torch.int32)
    order = torch.argsort(votes, dim=1, descending=True, stable=True)[:, :5]
    top5[:, :order.shape[1]] = order.to(torch.int32)
    return votes, top5


def hits_ref(top5, labels, K):
    """(top-1 hits, top-5 hits) of int64 `labels` against top5; a label outside [0, K) scores nothing."""
    ok = (labels >= 0) & (labels < K)
    h1 = ok & (top5[:, 0].long() == labels)
    h5 = ok & (top5.long() == labels[:, None]).any(1)
    return float(h1.sum()), float(h5.sum())


def normalize_ref(x, eps=1e-12):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(eps)


def knn_ref(bank, queries, bank_labels, K, k=20, T=0.07):
    """The whole pipeline in float64 -> dict(sim [Q, N], val, idx, votes, top5)."""
    sim = normalize_ref(queries) @ normalize_ref(bank).T
    val, idx = select_ref(sim, k)
    votes, top5 = vote_ref(val, idx, bank_labels, K, T)
    return dict(sim=sim, val=val, idx=idx, votes=votes, top5=top5)


def top1_margin(votes):
    """Relative gap between the largest and the second largest vote of every row (1 when there is one class only)."""
    s = torch.sort(votes, dim=1, descending=True).values
    if s.shape[1] < 2:
        return torch.ones(s.shape[0], dtype=s.dtype)
    return (s[:, 0] - s[:, 1]) / s[:, 0]


def ranks_separated(votes, rel=1e-3):
    """True when, in every row, two consecutive ranked votes either differ by more than `rel` relative or are exactly equal (identical inputs:
    the same weights added in the same order, or no vote at all) — then fp32 rounding cannot reorder the ranking."""
    s = torch.sort(votes, dim=1, descending=True).values
    a, b = s[:, :-1], s[:, 1:]
    return bool(((a == b) | ((a - b) > rel * a)).all())
