"""YotubeDNN (the reference's spelling) — drop-in for rec_pangu/models/sequence/yotubednn.py.

The model is nothing but the family's loss head behind a masked mean of the history's item rows:
    user_emb = mean_l(item_emb(hist)[b, l] * mask[b, l])         (divisor L, not the mask count: yotubednn.py:34-36)
    loss     = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
On the HIP device both are the library's kernels (Fh.hist_mean, Fh.full_softmax_ce): neither the [B, L, D] lookup nor any
[B, V] tensor is formed.  On the CPU the reference's torch formulas.

One deliberate difference: the target is taken as `.view(-1)`.  The reference's `.squeeze()` turns the target of a batch
of one into a 0-d tensor, and CrossEntropyLoss then raises "Expected input batch_size (1) to match target batch_size (0)";
here a batch of one trains.
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel


class YotubeDNN(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(YotubeDNN, self).__init__(enc_dict, config)
        self.reset_parameters()

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        mask = data['hist_mask_list']
        # while training one check covers both launches (they share the device flag): the loss makes it
        check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
        user_emb = Fh.hist_mean(self.item_emb.weight, item_seq, mask, check_indices=check)
        if is_training:
            item = data['target_item'].view(-1)
            loss = self.calculate_loss(user_emb, item)
            return {'user_emb': user_emb, 'loss': loss}
        return {'user_emb': user_emb}
