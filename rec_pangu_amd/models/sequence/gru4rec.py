"""GRU4Rec — drop-in for rec_pangu/models/sequence/gru4rec.py.

    user_emb = out(h_T),  h_T the top layer's state of a two-layer GRU (H = D, with biases) after the row's len = sum(mask)
    steps over item_emb(hist);  loss = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
On the HIP device: one recurrence launch per layer and direction (Fh.gru_encode: the item rows are gathered inside the first
layer's kernel, no [B, L, D] tensor; only the hidden states are kept for the backward), the library's Linear for `out` and
the family's fused loss head.  On the CPU the reference's torch formulas (pack / unpack).

Deliberate differences: the target is taken as `.view(-1)` (a batch of one trains, as in YotubeDNN); a row without history
gives a zero user_emb on the HIP device (the CPU path raises inside pack_padded_sequence like the reference).
"""
from typing import Dict

import torch

from ..base_model import SequenceBaseModel
from ..layers import GRU4RecEncoder


class GRU4Rec(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(GRU4Rec, self).__init__(enc_dict, config)
        self.gru = GRU4RecEncoder(self.embedding_dim, self.embedding_dim)
        self.reset_parameters()

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        item_seq_length = torch.sum(data['hist_mask_list'], dim=1)
        if item_seq.is_cuda:
            # while training one check covers the lookup and the loss (they share the device flag): the loss makes it
            check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
            user_emb = self.gru(None, item_seq_length, ids=item_seq, item_weight=self.item_emb.weight, check_indices=check)
        else:
            user_emb = self.gru(self.item_emb(item_seq), item_seq_length)
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
