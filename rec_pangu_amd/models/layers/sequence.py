"""Sequence poolings of the reference (rec_pangu/models/layers/sequence.py:13-59), its KMaxPooling (:63-86) and its
GRU4RecEncoder (:231-251) as drop-in modules.

On a HIP tensor they run rp_seq_pool_fwd / _bwd (one read of the [B, L, D] tensor); on the CPU the reference's own
formulas.  When the pooled tensor comes straight from a `_seq` lookup, `EmbeddingLayer.lookup_pooled` fuses lookup and
pooling and the [B, L, D] tensor never exists.
"""
import torch
from torch import nn

from ... import functional as Fh


class MaskedAveragePooling(nn.Module):
    """sum over dim 1 / (number of non-zero elements per (sample, column) + 1e-16) — sequence.py:30-36"""

    def forward(self, embedding_matrix: torch.Tensor) -> torch.Tensor:
        if embedding_matrix.is_cuda and embedding_matrix.dim() == 3:
            return Fh.seq_pool(embedding_matrix, "average")
        nonzero = embedding_matrix.ne(0).sum(dim=1).to(embedding_matrix.dtype)  # per (sample, column), like the reference
        return embedding_matrix.sum(dim=1) / (nonzero + 1e-16)


class MaskedSumPooling(nn.Module):
    """sum over dim 1 (padding rows count unless they are zero) — sequence.py:58-59"""

    def forward(self, embedding_matrix: torch.Tensor) -> torch.Tensor:
        if embedding_matrix.is_cuda and embedding_matrix.dim() == 3:
            return Fh.seq_pool(embedding_matrix, "sum")
        return embedding_matrix.sum(dim=1)


class KMaxPooling(nn.Module):
    """the k largest entries along `dim`, in their original order — sequence.py:63-86 (topk -> sort the indices -> gather).
    CCPM's conv stack runs it inside rp_ccpm_fwd / rp_ccpm_bwd (functional.ccpm_conv_stack); used on its own on a HIP
    tensor this module composes it from device ops (counted).  torch leaves topk's order among exact ties unspecified."""

    def __init__(self, k: int, dim: int):
        super(KMaxPooling, self).__init__()
        self.k = k
        self.dim = dim

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        if X.is_cuda:
            from ... import hip
            hip.note_torch_path("KMaxPooling called on its own (the kernels run CCPM's whole conv stack: "
                                "functional.ccpm_conv_stack)")
        index = X.topk(self.k, dim=self.dim)[1].sort(dim=self.dim)[0]
        return X.gather(self.dim, index)


class GRU4RecEncoder(nn.Module):
    """out(hidden[-1]) of a multi-layer nn.GRU run over each row's first `lengths[b]` positions — sequence.py:231-251, the same
    constructor, parameter names (`rnn.*`, `out.weight`) and registration order.  `rnn` is a real nn.GRU: it holds the
    parameters (state_dict keys, shapes and the init RNG stream are the reference's) and runs the CPU path; on the HIP device
    the recurrence kernels read its parameters (Fh.gru_encode), the readout is the library's Linear.  The reference's sort by
    length and its inverse cancel and are gone.

    forward(seq, lengths) as in the reference, or forward(None, lengths, ids=..., item_weight=...) to have the item rows
    gathered inside the first layer's kernel.  A row of length 0: the CPU path raises inside pack_padded_sequence like the
    reference; the HIP path gives a zero row."""

    def __init__(self, emb_size, hidden_size=128, num_layers=2):
        super().__init__()
        self.rnn = nn.GRU(input_size=emb_size, hidden_size=hidden_size, num_layers=num_layers, batch_first=True)
        self.out = nn.Linear(hidden_size, emb_size, bias=False)

    def forward(self, seq, lengths, ids=None, item_weight=None, check_indices: str = "sync"):
        steps = lengths.to(torch.int64)
        _, hidden = Fh.gru_encode(self.rnn, steps, steps - 1, x=seq, ids=ids, item_weight=item_weight, packed=True,
                                  check_indices=check_indices)
        if hidden.is_cuda:
            return Fh.linear_act(hidden, self.out.weight)
        return self.out(hidden)
