"""NISER — drop-in for rec_pangu/models/sequence/niser.py (config keys and defaults as there: step 1, item_dropout 0.1).

SRGNN with normalised embeddings: the node rows go through item_dropout, then F.normalize(dim=-1), before the cell;
pos_embedding.weight[:L] is added to seq_hidden BEFORE ht is taken (ht carries its position); the readout is SRGNN's;
F.normalize is applied to the result.
On the HIP device SRGNN's launches plus Fh.dropout (the library's Philox stream) and Fh.l2_normalize on both sides, and
Fh.seq_take for ht.  On the CPU the same formulas in torch ops; no dgl anywhere.

Deliberate differences: SRGNN's (models/sequence/srgnn.py), with one change: ht is the row at sum(hist_mask_list) - 1 of
seq_hidden + positions, zero for a sample without history (on the CPU too: nothing raises).
"""
from typing import Dict

import torch
from torch import nn

from ... import functional as Fh
from ..layers.graph import SRGNNCell
from .srgnn import SRGNN


class NISER(SRGNN):
    def __init__(self, enc_dict, config):
        super(SRGNN, self).__init__(enc_dict, config)  # (SequenceBaseModel's: the submodules are created in NISER's own order)

        self.step = self.config.get('step', 1)

        self.pos_embedding = nn.Embedding(self.max_length, self.embedding_dim)
        self.item_dropout = nn.Dropout(config.get('item_dropout', 0.1))

        self.gnncell = SRGNNCell(self.embedding_dim)
        self.linear_one = nn.Linear(self.embedding_dim, self.embedding_dim)
        self.linear_two = nn.Linear(self.embedding_dim, self.embedding_dim)
        self.linear_three = nn.Linear(self.embedding_dim, 1, bias=False)
        self.linear_transform = nn.Linear(self.embedding_dim * 2, self.embedding_dim)

        self.reset_parameters()

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        mask = data['hist_mask_list']
        item_seq_len = (mask != 0).sum(dim=1)
        alias, hidden = self.node_rows(item_seq, is_training)
        if hidden.is_cuda:
            if self.training and self.item_dropout.p > 0:
                hidden = Fh.dropout(hidden, self.item_dropout.p)
        else:
            hidden = self.item_dropout(hidden)
        hidden = Fh.l2_normalize(hidden)
        seq_hidden, _ = self.gnncell.encode(alias, hidden, self.step)
        seq_hidden = seq_hidden + self.pos_embedding.weight[:seq_hidden.shape[1]].unsqueeze(0)
        if seq_hidden.is_cuda:
            ht = Fh.seq_take(seq_hidden, item_seq_len - 1)
        else:
            ht = self.gather_indexes(seq_hidden, (item_seq_len - 1).clamp(min=0)) * (item_seq_len > 0).unsqueeze(-1)
        user_emb = Fh.l2_normalize(self.readout(seq_hidden, ht, mask))
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
