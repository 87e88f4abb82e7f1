"""GCSAN — drop-in for rec_pangu/models/sequence/gcsan.py (config keys and defaults as there: n_layers 2, n_heads 4,
hidden_size 64, inner_size 32, hidden_dropout_prob / attn_dropout_prob 0.1, hidden_act 'gelu', layer_norm_eps 0.001, step 1,
weight 0.1; hidden_size is the encoder's width and has to equal embedding_dim, as there).

    seq_hidden, ht = SRGNN's session-graph encoder (models/sequence/srgnn.py)
    at       = TransformerEncoder(seq_hidden, causal + padding mask)[-1][b, len_b - 1]
    user_emb = weight * at + (1 - weight) * ht
On the HIP device the graph and cell launches of SRGNN, then TransformerEncoder.encode_last (the final layer runs for the one
row per sample that is read) and the family's fused loss head.  On the CPU the reference's torch formulas; no dgl anywhere.

As in the reference: linear_one, linear_two, linear_three and linear_transform are created, initialised and in the
state_dict, and never used: they take no gradient.

Deliberate differences: SRGNN's (models/sequence/srgnn.py); a sample without history gives at = ht = 0, hence user_emb = 0
(on the CPU too: nothing raises).
"""
from typing import Dict

import torch
from torch import nn

from ..layers.graph import SRGNNCell
from ..layers.transformer import TransformerEncoder
from .srgnn import SRGNN


class GCSAN(SRGNN):
    def __init__(self, enc_dict, config):
        super(SRGNN, self).__init__(enc_dict, config)  # (SequenceBaseModel's: the submodules are created in GCSAN's own order)

        self.n_layers = config.get('n_layers', 2)
        self.n_heads = config.get('n_heads', 4)
        self.hidden_size = config.get('hidden_size', 64)  # same as embedding_size
        self.inner_size = config.get('inner_size', 32)  # the dimensionality in feed-forward layer
        self.hidden_dropout_prob = config.get('hidden_dropout_prob', 0.1)
        self.attn_dropout_prob = config.get('attn_dropout_prob', 0.1)
        self.hidden_act = config.get('hidden_act', 'gelu')
        self.layer_norm_eps = config.get('layer_norm_eps', 0.001)
        self.step = config.get('step', 1)
        self.weight = config.get('weight', 0.1)

        self.gnncell = SRGNNCell(self.embedding_dim)
        self.linear_one = nn.Linear(self.embedding_dim, self.embedding_dim)
        self.linear_two = nn.Linear(self.embedding_dim, self.embedding_dim)
        self.linear_three = nn.Linear(self.embedding_dim, 1, bias=False)
        self.linear_transform = nn.Linear(self.embedding_dim * 2, self.embedding_dim)

        self.self_attention = TransformerEncoder(
            n_layers=self.n_layers,
            n_heads=self.n_heads,
            hidden_size=self.hidden_size,
            inner_size=self.inner_size,
            hidden_dropout_prob=self.hidden_dropout_prob,
            attn_dropout_prob=self.attn_dropout_prob,
            hidden_act=self.hidden_act,
            layer_norm_eps=self.layer_norm_eps
        )

        self.reset_parameters()

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        mask = data['hist_mask_list']
        alias, hidden = self.node_rows(item_seq, is_training)
        seq_hidden, ht = self.gnncell.encode(alias, hidden, self.step)
        if seq_hidden.is_cuda:
            at = self.self_attention.encode_last(seq_hidden, mask)
        else:
            item_seq_len = torch.sum(mask, dim=-1).long()
            attention_mask = self.get_attention_mask(mask)
            output = self.self_attention(seq_hidden, attention_mask, output_all_encoded_layers=True)[-1]
            at = self.gather_indexes(output, (item_seq_len - 1).clamp(min=0)) * (item_seq_len > 0).unsqueeze(-1)
        user_emb = self.weight * at + (1 - self.weight) * ht
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
