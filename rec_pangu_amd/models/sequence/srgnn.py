"""SRGNN — drop-in for rec_pangu/models/sequence/srgnn.py (config key and default as there: step 1).

    nodes, alias = the session graph of every sample (Fh.session_graph: distinct items ascending, one transition per
                   consecutive pair of items, repeated transitions counted as often as they occur)
    hidden       = `step` rounds of SRGNNCell over item_emb(nodes)
    seq_hidden[b, l] = hidden[b, alias[b, l]],  ht = seq_hidden[b, n_b - 1]
    alpha    = linear_three(sigmoid(linear_one(ht) + linear_two(seq_hidden)))
    user_emb = linear_transform(cat[sum_l alpha * seq_hidden * mask, ht])
    loss     = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
On the HIP device: one rp_session_graph launch -> Fh.hist_rows over the node ids -> one fused cell launch per step and
direction (csrc/session_graph.hip), the last one reading seq_hidden and ht back -> linear_one / linear_two on
the library's Linear -> Fh.narm_attention (linear_three has no bias, so NARM's readout with hist_mask_list as its ids is this
formula) -> linear_transform -> the family's fused loss head.  On the CPU the same formulas in torch ops; no dgl anywhere.

Deliberate differences:
  - the target is taken as `.view(-1)` (a batch of one trains), as in the rest of the family;
  - seq_hidden is ZERO at padded positions (the reference reads the first sample's node 0 there; no output or gradient
    depends on those rows: the mask multiplies them);
  - ht is read at the last item with id > 0; a sample without history gives ht = 0, hence a defined user_emb, and takes no
    gradient through the encoder; a sample of one item has no transition, in = out = 0, and the cell still runs (the
    reference raises when such a sample is the LAST of the batch: dgl infers the node count from the edges);
  - step must be at least 1.
"""
from typing import Dict

import torch
from torch import nn

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers.graph import SRGNNCell


class SRGNN(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(SRGNN, self).__init__(enc_dict, config)

        self.step = self.config.get('step', 1)

        self.gnncell = SRGNNCell(self.embedding_dim)
        self.linear_one = nn.Linear(self.embedding_dim, self.embedding_dim)
        self.linear_two = nn.Linear(self.embedding_dim, self.embedding_dim)
        self.linear_three = nn.Linear(self.embedding_dim, 1, bias=False)
        self.linear_transform = nn.Linear(self.embedding_dim * 2, self.embedding_dim)

        self.reset_parameters()

    def node_rows(self, item_seq, is_training):
        """-> (alias int32 [B, L], item_emb over the node ids [B, L, D])"""
        nodes, alias = Fh.session_graph(item_seq)[:2]
        if item_seq.is_cuda:
            # while training one check covers the lookup and the loss (they share the device flag): the loss makes it
            check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
            return alias, Fh.hist_rows(self.item_emb.weight, nodes, check_indices=check)
        return alias, self.item_emb(nodes)

    def readout(self, seq_hidden, ht, mask):
        """SRGNN's additive attention over seq_hidden against ht -> linear_transform(cat[a, ht])"""
        if seq_hidden.is_cuda:
            q1 = Fh.linear_act(ht, self.linear_one.weight, self.linear_one.bias)
            q2 = Fh.linear_act(seq_hidden, self.linear_two.weight, self.linear_two.bias)
            c = Fh.narm_attention(q2, q1, self.linear_three.weight, (mask != 0).to(torch.int64), seq_hidden, ht)
            return Fh.linear_act(c, self.linear_transform.weight, self.linear_transform.bias)
        q1 = self.linear_one(ht).view(ht.size(0), 1, ht.size(1))
        q2 = self.linear_two(seq_hidden)
        alpha = self.linear_three(torch.sigmoid(q1 + q2))
        a = torch.sum(alpha * seq_hidden * (mask != 0).view(seq_hidden.size(0), -1, 1).float(), 1)
        return self.linear_transform(torch.cat([a, ht], dim=1))

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        alias, hidden = self.node_rows(item_seq, is_training)
        seq_hidden, ht = self.gnncell.encode(alias, hidden, self.step)
        user_emb = self.readout(seq_hidden, ht, data['hist_mask_list'])
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
