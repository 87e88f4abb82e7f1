"""Sequence poolings of the reference (rec_pangu/models/layers/sequence.py:13-59), its KMaxPooling (:63-86), its
GRU4RecEncoder (:231-251), its STAMPLayer (:89-144) and its BERT4RecEncoder with the MultiHeadAttention and TransformerLayer
under it (:150-228, :286-312) as drop-in modules.

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


class MultiHeadAttention(nn.Module):
    """The projections and the attention of the reference's sequence.py:150-197 (no output projection): the same constructor
    and the parameters `q_linear` (absent with kq_same), `k_linear`, `v_linear` in that order.  Not the class of the same
    name in layers/transformer.py (SASRec's), as in the reference.

    forward(q, k, v, mask): mask None, anything that broadcasts against the [B, heads, Lq, Lk] scores (the reference's
    [B, 1, 1, L] key-padding mask) or a [B, L] content mask (non-zero = content).  Self-attention (q, k and v the same
    tensor) under a [B, L] mask on the HIP device is one stacked Q | K | V GEMM and Fh.seq_attention(causal=False): one
    launch each way, nothing of size L x L stored; qpos (int64 [B], that path only) selects one query row per sample ->
    [B, D].  Everything else runs the torch formulas (counted on the HIP device).

    Deliberate difference: the reference subtracts the maximum score of the WHOLE batch tensor before the softmax
    (`scores - scores.max()`); here the maximum is subtracted per row.  Equal unless a row's own maximum lies about 87 below
    the batch's, where the reference's row collapses to 0.  A row without a content key is 0 (the reference: NaN -> 0) and
    passes zero gradients (the reference: NaN)."""

    def __init__(self, d_model, n_heads, kq_same=False, bias=True):
        super().__init__()
        self.d_model = d_model
        self.h = n_heads
        self.d_k = self.d_model // self.h
        self.kq_same = kq_same

        if not kq_same:
            self.q_linear = nn.Linear(d_model, d_model, bias=bias)
        self.k_linear = nn.Linear(d_model, d_model, bias=bias)
        self.v_linear = nn.Linear(d_model, d_model, bias=bias)

    def head_split(self, x):  # bs * h * seq_len * d_k
        new_x_shape = x.size()[:-1] + (self.h, self.d_k)
        return x.view(*new_x_shape).transpose(-2, -3)

    @staticmethod
    def scaled_dot_product_attention(q, k, v, d_k, mask=None):
        scores = torch.matmul(q, k.transpose(-2, -1)) / d_k ** 0.5  # bs, head, q_len, k_len
        if mask is not None:
            scores = scores.masked_fill(mask == 0, float("-inf"))
        top = scores.detach().max(dim=-1, keepdim=True).values
        e = torch.exp(scores - torch.where(torch.isinf(top), torch.zeros_like(top), top))
        den = e.sum(dim=-1, keepdim=True)
        return torch.matmul(e / torch.where(den > 0, den, torch.ones_like(den)), v)

    def _linears(self):
        return [self.k_linear if self.kq_same else self.q_linear, self.k_linear, self.v_linear]

    def forward(self, q, k, v, mask=None, qpos=None):
        fused = q.is_cuda and q is k and k is v and mask is not None and mask.dim() == 2 and q.dim() == 3
        if not fused:
            if qpos is not None:
                raise ValueError("MultiHeadAttention: qpos needs self-attention under a [B, L] content mask on the HIP device")
            if q.is_cuda:
                Fh.hip.note_torch_path("sequence.MultiHeadAttention outside self-attention under a [B, L] content mask")
            if mask is not None and mask.dim() == 2 and q.dim() == 3:
                mask = mask.view(mask.shape[0], 1, 1, mask.shape[1])
            origin_shape = q.size()
            q = self.head_split((self.k_linear if self.kq_same else self.q_linear)(q))
            k = self.head_split(self.k_linear(k))
            v = self.head_split(self.v_linear(v))
            output = self.scaled_dot_product_attention(q, k, v, self.d_k, mask)
            return output.transpose(-2, -3).reshape(origin_shape)
        B, L, D = q.shape
        rows = q.reshape(B * L, D)
        lin = self._linears()
        has_bias = self.k_linear.bias is not None

        def stacked(ms):
            return Fh.stack_rows([m.weight for m in ms]), (Fh.stack_rows([m.bias.view(-1, 1) for m in ms]).view(-1) if has_bias
                                                           else None)

        if qpos is None:
            qkv = Fh.linear_act(rows, *stacked(lin))
            return Fh.seq_attention(qkv, mask, self.h, causal=False).reshape(B, L, D)
        kv = Fh.linear_act(rows, *stacked(lin[1:]))
        qrow = Fh.linear_act(Fh.seq_take(q, qpos), lin[0].weight, lin[0].bias)
        return Fh.seq_attention(kv, mask, self.h, qpos=qpos, q=qrow, causal=False)


class TransformerLayer(nn.Module):
    """The block of the reference's sequence.py:200-228: the attention above, residual + LayerNorm, a ReLU feed-forward of
    width d_ff, residual + LayerNorm; LayerNorm eps is torch's default, dropout defaults to 0.  The same constructor, names
    and registration order (`masked_attn_head`, `layer_norm1`, `dropout1`, `linear1`, `linear2`, `layer_norm2`, `dropout2`).
    Not layers/transformer.py's class of the same name.

    forward(seq, mask): mask as MultiHeadAttention's.  Under a [B, L] content mask on the HIP device the attention is the
    fused one and the rest runs on the library's Linear and LayerNorm; with qpos (int64 [B]) everything after K and V runs
    for the one selected row per sample -> [B, D]."""

    def __init__(self, d_model, d_ff, n_heads, dropout=0, kq_same=False):
        super().__init__()
        self.masked_attn_head = MultiHeadAttention(d_model, n_heads, kq_same=kq_same)

        self.layer_norm1 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)

        self.linear1 = nn.Linear(d_model, d_ff)
        self.linear2 = nn.Linear(d_ff, d_model)

        self.layer_norm2 = nn.LayerNorm(d_model)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, seq, mask=None, qpos=None):
        if not (seq.is_cuda and mask is not None and mask.dim() == 2):
            context = self.masked_attn_head(seq, seq, seq, mask)
            context = self.layer_norm1(self.dropout1(context) + seq)
            output = self.linear1(context).relu()
            output = self.linear2(output)
            return self.layer_norm2(self.dropout2(output) + context)
        drop = self.training and self.dropout1.p > 0
        context = self.masked_attn_head(seq, seq, seq, mask, qpos=qpos)
        residual = seq if qpos is None else Fh.seq_take(seq, qpos)
        shape = context.shape
        context, residual = context.reshape(-1, shape[-1]), residual.reshape(-1, shape[-1])
        if drop:
            context = Fh.dropout(context, self.dropout1.p)
        context = Fh.layer_norm(context + residual, self.layer_norm1)
        output = Fh.linear_act(context, self.linear1.weight, self.linear1.bias, act=Fh.ACT_RELU)
        output = Fh.linear_act(output, self.linear2.weight, self.linear2.bias)
        if drop:
            output = Fh.dropout(output, self.dropout2.p)
        return Fh.layer_norm(output + context, self.layer_norm2).reshape(shape)


class BERT4RecEncoder(nn.Module):
    """Bidirectional self-attention over the first lengths[b] positions of each row, read at position lengths[b] - 1 —
    sequence.py:286-312 of the reference: the same constructor, `p_embeddings` then `transformer_block.{i}.*`.  Padded
    positions take position row 0 (the reference's `len_range * valid_mask`).

    On the HIP device: the position rows as a select between `p_embeddings.weight[:L]` and its row 0, per layer one stacked Q | K | V GEMM and the key-padding
    attention under mask = arange(L) < lengths; the FINAL layer runs in last-row mode at qpos = lengths - 1.  On the CPU the
    reference's formulas (with MultiHeadAttention's per-row maximum).  A row of length 0 gives a zero vector on both paths
    (the reference reads position -1 of the masked output: 0 as well)."""

    def __init__(self, emb_size, max_his, num_layers=2, num_heads=2):
        super().__init__()
        self.p_embeddings = nn.Embedding(max_his + 1, emb_size)
        self.transformer_block = nn.ModuleList([
            TransformerLayer(d_model=emb_size, d_ff=emb_size, n_heads=num_heads)
            for _ in range(num_layers)
        ])

    def forward(self, seq, lengths):
        batch_size, seq_len = seq.size(0), seq.size(1)
        lengths = lengths.to(torch.int64)
        len_range = torch.arange(seq_len, device=seq.device)
        valid_mask = len_range[None, :] < lengths[:, None]
        position = len_range[None, :] * valid_mask.long()
        if not seq.is_cuda or len(self.transformer_block) == 0:
            seq = seq + self.p_embeddings(position)
            attn_mask = valid_mask.view(batch_size, 1, 1, seq_len)
            for block in self.transformer_block:
                seq = block(seq, attn_mask)
            seq = seq * valid_mask[:, :, None].to(seq.dtype)
            return seq[torch.arange(batch_size, device=seq.device), lengths - 1]
        # position[b, l] is l inside the row and 0 behind it: a select between two broadcasts instead of a lookup, whose
        # backward would have ONE writer walk the B L / 2 occurrences of row 0 in order (20 ms at B = 4096, L = 20)
        w = self.p_embeddings.weight
        seq = seq + torch.where(valid_mask.unsqueeze(-1), w[:seq_len].unsqueeze(0), w[0].view(1, 1, -1))
        content = valid_mask.to(torch.float32)
        for block in self.transformer_block[:-1]:
            seq = block(seq, content)
        last = lengths - 1
        out = self.transformer_block[-1](seq, content, qpos=last)
        return out * (last >= 0).to(out.dtype).view(-1, 1)
