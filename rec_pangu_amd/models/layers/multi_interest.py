"""MultiInterestSelfAttention — drop-in for rec_pangu/models/layers/multi_interest.py:11-53, ComirecSA's encoder (below) — and
CapsuleNetwork — drop-in for rec_pangu/models/layers/multi_interest.py:56-161: the multi-interest encoder of MIND
(bilinear_type 0) and ComirecDR (bilinear_type 2).  The same constructor, attributes and state_dict keys (`relu.0.weight`
exists even when relu_layer is off; `linear.weight` for types 0 / 1, `w` [1, L, K D, D] for type 2).

    u_hat = linear(item_eb)                         type 0: [B, L, D], read by all K interests; type 1: [B, L, K D]
          = sum_d w[s, n, d] item_eb[b, s, d]       type 2: [B, L, K D], every position its own matrix
    interests = three rounds of dynamic routing over u_hat (Fh.capsule_route), optionally relu(Linear(.))

On the HIP device: types 0 / 1 project through the library's Linear over the [B L, D] rows, type 2 through one launch for
all positions (Fh.capsule_project: the reference's [B, L, K D, D] product is never formed); the routing is one launch each
way and reads type 0's rows with interest stride 0 (the reference's .repeat(1, 1, K) does not exist).  On the CPU the
reference's torch formulas, op for op.

MIND's random initial routing logits are drawn in `initial_logits`, where the reference draws them (in evaluation too), so
the generator's stream is the reference's; tests replace the method to feed recorded logits.
"""
import torch
from torch import nn

from ... import functional as Fh


class MultiInterestSelfAttention(nn.Module):
    """A = softmax over positions of tanh(x W1) W2 (masked positions at -1e9), interests = A^T x  [B, K, D].  The same
    constructor and parameters W1 [D, d], W2 [d, K], W3 [D, D] in that order, drawn with torch.rand as the reference does
    (the generator's stream); W3 exists, is initialised and is in the state_dict, and nothing reads it: its grad stays None.
    The whole forward is one Fh.attention_pool node (csrc/attn_pool.hip): on the HIP device the hidden tensor
    [B, L, d] (four times the input at the default d = 4 D) exists on neither side."""

    def __init__(self, embedding_dim: int, num_attention_heads: int, d: int = None) -> None:
        super(MultiInterestSelfAttention, self).__init__()
        self.embedding_dim = embedding_dim
        self.num_attention_heads = num_attention_heads
        if d is None:
            self.d = self.embedding_dim * 4
        else:
            self.d = d

        self.W1 = nn.Parameter(torch.rand(self.embedding_dim, self.d), requires_grad=True)
        self.W2 = nn.Parameter(torch.rand(self.d, self.num_attention_heads), requires_grad=True)
        self.W3 = nn.Parameter(torch.rand(self.embedding_dim, self.embedding_dim), requires_grad=True)

    def forward(self, sequence_embeddings: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
        """sequence_embeddings [B, L, D]; mask [B, L, 1] or [B, L] of 0 / 1, None: every position counts"""
        B, L, _ = sequence_embeddings.shape
        if mask is None:
            valid = torch.ones(B, L, dtype=sequence_embeddings.dtype, device=sequence_embeddings.device)
        else:
            valid = mask.reshape(B, L)
        return Fh.attention_pool(sequence_embeddings, self.W1, self.W2, valid, act="tanh", norm="softmax")


class CapsuleNetwork(nn.Module):
    def __init__(self, hidden_size: int, seq_len: int, bilinear_type: int = 2, interest_num: int = 4,
                 routing_times: int = 3, hard_readout: bool = True, relu_layer: bool = False) -> None:
        super(CapsuleNetwork, self).__init__()
        self.hidden_size = hidden_size  # h
        self.seq_len = seq_len  # s
        self.bilinear_type = bilinear_type
        self.interest_num = interest_num
        self.routing_times = routing_times
        self.hard_readout = hard_readout
        self.relu_layer = relu_layer
        self.stop_grad = False
        self.relu = nn.Sequential(
            nn.Linear(self.hidden_size, self.hidden_size, bias=False),
            nn.ReLU()
        )
        if self.bilinear_type == 0:  # MIND
            self.linear = nn.Linear(self.hidden_size, self.hidden_size, bias=False)
        elif self.bilinear_type == 1:
            self.linear = nn.Linear(self.hidden_size, self.hidden_size * self.interest_num, bias=False)
        else:  # ComiRec_DR
            self.w = nn.Parameter(torch.Tensor(1, self.seq_len, self.interest_num * self.hidden_size, self.hidden_size))

    def initial_logits(self, batch: int, device) -> torch.Tensor:
        """MIND's Gaussian initial routing logits [B, K, L] (multi_interest.py:122-123)"""
        return torch.randn(batch, self.interest_num, self.seq_len, device=device, requires_grad=False)

    def forward(self, item_eb, mask, device):
        if item_eb.shape[1] != self.seq_len:
            raise ValueError(f"CapsuleNetwork: the history has {item_eb.shape[1]} positions, seq_len is {self.seq_len}")
        on_hip = item_eb.is_cuda
        if self.bilinear_type in (0, 1):
            item_eb_hat = Fh.linear_act(item_eb, self.linear.weight) if on_hip else self.linear(item_eb)
        else:
            item_eb_hat = Fh.capsule_project(item_eb, self.w)
        b0 = self.initial_logits(item_eb.shape[0], device) if self.bilinear_type == 0 else None
        interest_capsule = Fh.capsule_route(item_eb_hat, mask, self.interest_num, b0=b0, shared=self.bilinear_type == 0,
                                            stop_grad=self.stop_grad, rounds=self.routing_times)
        if self.relu_layer:  # (MIND on the book data set)
            if on_hip:
                interest_capsule = Fh.linear_act(interest_capsule, self.relu[0].weight, act=Fh.ACT_RELU)
            else:
                interest_capsule = self.relu(interest_capsule)
        return interest_capsule
