"""Sequence poolings of the reference (rec_pangu/models/layers/sequence.py:13-59), its KMaxPooling (:63-86) and its
GRU4RecEncoder (:231-251) and its STAMPLayer (:89-144) as drop-in modules.

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


class STAMPLayer(nn.Module):
    """STAMP's readout — sequence.py:89-144, the same constructor and the reference's six Linears under the same names in
    the same creation order.  With valid = (position < lens):

        m_s = sum_l valid x_l / lens,  x_t = x[lens - 1]
        alpha_l = valid attn_e(sigmoid(attn_i(x_l) + attn_t(x_t) + attn_s(m_s))),  m_a = sum_l alpha_l x_l
        sr = fc_a(m_a) * fc_t(x_t)

    forward(emb_seqs, lens) as in the reference (feat_drop applied here); forward(emb_seqs, lens, m_s=...) takes the mean
    from the caller and applies no dropout (STAMP's device path draws the rows' dropout itself and reads the mean off the
    table when there is none).  On the HIP device attn_t / attn_s / fc_a / fc_t run on the library's Linear, attn_i and
    attn_e inside ONE Fh.attention_pool node (csrc/attn_pool.hip) whose mask mode gives the rows at
    valid = 0 weight 0: the reference's masked_fill of the rows needs no copy.

    Deliberate difference: lens = 0 gives m_s = x_t = 0 and m_a = 0, hence sr = fc_a.bias * fc_t.bias, and no gradient
    reaches the rows (the reference divides by zero: NaN)."""

    def __init__(self, embedding_dim: int, feat_drop: float = 0.0):
        super().__init__()
        self.feat_drop = nn.Dropout(feat_drop) if feat_drop > 0 else None
        self.fc_a = nn.Linear(embedding_dim, embedding_dim, bias=True)
        self.fc_t = nn.Linear(embedding_dim, embedding_dim, bias=True)
        self.attn_i = nn.Linear(embedding_dim, embedding_dim, bias=False)
        self.attn_t = nn.Linear(embedding_dim, embedding_dim, bias=True)
        self.attn_s = nn.Linear(embedding_dim, embedding_dim, bias=False)
        self.attn_e = nn.Linear(embedding_dim, 1, bias=False)

    def forward(self, emb_seqs: torch.Tensor, lens: torch.Tensor, m_s: torch.Tensor = None) -> torch.Tensor:
        on_hip = emb_seqs.is_cuda
        if m_s is None and self.feat_drop is not None:
            if on_hip:
                if self.training:
                    emb_seqs = Fh.dropout(emb_seqs, self.feat_drop.p)
            else:
                emb_seqs = self.feat_drop(emb_seqs)
        batch_size, max_len, _ = emb_seqs.size()
        valid = (torch.arange(max_len, device=lens.device).unsqueeze(0) < lens.unsqueeze(-1)).to(emb_seqs.dtype)
        some = (lens > 0).to(emb_seqs.dtype).unsqueeze(-1)
        if on_hip:
            if m_s is None:
                m_s = Fh.seq_pool(emb_seqs * valid.unsqueeze(-1), "sum") / lens.clamp(min=1).unsqueeze(-1)
            xt = Fh.seq_take(emb_seqs, lens.to(torch.int64) - 1)  # (a zero row where lens = 0)
            c = Fh.linear_act(xt, self.attn_t.weight, self.attn_t.bias) + Fh.linear_act(m_s, self.attn_s.weight)
        else:
            if m_s is None:
                m_s = (emb_seqs * valid.unsqueeze(-1)).sum(dim=1) / lens.clamp(min=1).unsqueeze(-1)
            xt = emb_seqs[torch.arange(batch_size), (lens - 1).clamp(min=0)] * some
            c = self.attn_t(xt) + self.attn_s(m_s)
        ma = Fh.attention_pool(emb_seqs, self.attn_i.weight.t(), self.attn_e.weight.t(), valid, bias=c, act="sigmoid",
                               norm="mask").squeeze(1)
        if on_hip:
            return Fh.linear_act(ma, self.fc_a.weight, self.fc_a.bias) * Fh.linear_act(xt, self.fc_t.weight, self.fc_t.bias)
        return self.fc_a(ma) * self.fc_t(xt)
