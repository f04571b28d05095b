"""Nearest-neighbour search and the weighted k-NN vote over a bank of features kept on the device (main_knn.py).

The bank is normalised once (ops.l2_normalize) into bf16 — or fp32 for exact work.  A search walks query chunks x bank chunks: one ops.gemm of the
normalised queries against the bank chunk (the bank is [N, D], which is the `b` operand's [N, K] layout: no transpose) into ONE reused fp32 tile,
then ops.knn_select merges that tile into the running best-k lists.  The chunk sizes bound memory: the full similarity matrix never exists.
bf16 operands go straight to an fp32 tile (csmae_gemm takes a c_dtype of its own), so there is no bf16 tile and no cast pass.  Everything is
enqueued on torch's current stream; nothing is read back."""
import torch

from . import ops


def _check_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("csmae_hip.knn needs GPU tensors: the MI355X path has no CPU fallback")


class KnnIndex:
    """features [N, D] fp32 and labels [N] int64 on the GPU -> a normalised bank in `dtype`.  `counts` [2] collects the top-1 / top-5 hits of
    every classify() call that is given labels (reset it with counts.zero_())."""

    def __init__(self, features, labels, num_classes, dtype=torch.bfloat16):
        _check_cuda(features, labels)
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"KnnIndex: dtype {dtype} is neither bfloat16 nor float32")
        N, D = features.shape
        if dtype == torch.bfloat16 and D % 8:
            raise ValueError(f"KnnIndex: the bf16 GEMM reads 8 features at a time: D = {D} is not a multiple of 8 (use dtype=torch.float32)")
        assert labels.shape == (N,) and labels.dtype == torch.int64
        self.N, self.D, self.num_classes, self.dtype = N, D, int(num_classes), dtype
        # rows padded with zeros to a multiple of 4: a GEMM's N is a multiple of 4, the select never reads the padding columns
        self.bank = torch.zeros((N + 3) // 4 * 4, D, device=features.device, dtype=dtype)
        ops.l2_normalize(features.float(), self.bank[:N])
        self.labels = labels.contiguous()
        self.counts = torch.zeros(2, device=features.device, dtype=torch.float32)
        self._scratch = {}

    def _buf(self, name, shape, dtype):
        """A scratch tensor that is kept between calls and only ever grows."""
        n = 1
        for s in shape:
            n *= s
        t = self._scratch.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = self._scratch[name] = torch.empty(n, device=self.bank.device, dtype=dtype)
        return t[:n].view(*shape)

    def search(self, queries, k, q_chunk=4096, b_chunk=8192):
        """queries [Q, D] fp32 -> (val [Q, k] fp32, idx [Q, k] int32): each query's k most similar bank rows by cosine similarity, descending, ties to
        the lower bank index, (-inf, -1) behind the N-th when the bank is smaller than k.  The result tensors are scratch of this index: the next
        search overwrites them."""
        _check_cuda(queries)
        Q, D = queries.shape
        assert D == self.D and q_chunk > 0 and b_chunk > 0
        b_chunk = (b_chunk + 3) // 4 * 4
        qn = self._buf("qn", (Q, D), self.dtype)
        ops.l2_normalize(queries.float(), qn)
        val = self._buf("val", (Q, k), torch.float32).fill_(float("-inf"))
        idx = self._buf("idx", (Q, k), torch.int32).fill_(-1)
        sim = self._buf("sim", (min(q_chunk, Q), min(b_chunk, self.bank.shape[0])), torch.float32)
        for q0 in range(0, Q, q_chunk):
            q1 = min(q0 + q_chunk, Q)
            for b0 in range(0, self.N, b_chunk):
                nb = min(b_chunk, self.N - b0)
                nb4 = (nb + 3) // 4 * 4
                tile = sim[:q1 - q0, :nb4]
                ops.gemm(qn[q0:q1], self.bank[b0:b0 + nb4], tile)
                ops.knn_select(tile, val[q0:q1], idx[q0:q1], base=b0, Bc=nb)
        return val, idx

    def classify(self, queries, k=20, T=0.07, labels=None, **chunks):
        """-> (top5 [Q, 5] int32, votes [Q, num_classes] fp32) of the weighted vote; with `labels` (int64 [Q]) the hits are added to self.counts."""
        _check_cuda(queries, labels)
        val, idx = self.search(queries, k, **chunks)
        Q = queries.shape[0]
        top5 = self._buf("top5", (Q, 5), torch.int32)
        votes = self._buf("votes", (Q, self.num_classes), torch.float32)
        ops.knn_vote(val, idx, self.labels, self.num_classes, T, top5, votes=votes, counts=self.counts,
                     query_labels=None if labels is None else labels.contiguous(), accumulate_counts=True)
        return top5, votes
