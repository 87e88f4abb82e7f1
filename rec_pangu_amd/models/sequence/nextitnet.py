"""NextItNet — drop-in for rec_pangu/models/sequence/nextitnet.py (config keys and defaults as there: dilations None,
one_masked False, kernel_size 3, feat_drop 0).

    len_b    = sum(hist_mask_list[b])                 (a prefix length: holes in the mask do not matter)
    user_emb = NextItNetLayer(item_emb(hist) with positions >= len_b zeroed)[b, :, len_b - 1]
    loss     = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
On the HIP device: Fh.hist_rows -> one fused launch per residual block and direction (the final block for the one row per
sample that is read: csrc/causal_conv.hip) -> the family's fused loss head.  On the CPU the reference's
torch formulas.

As in the reference: `fc` is created and never used (it is in the state_dict, takes its draws from the init stream and
never gets a gradient); reset_parameters() Kaiming-initialises gamma and beta too (they are 3-D); a row without history
does not raise, its user_emb is the value at position L - 1 of an all-zero input.

Deliberate differences:
  - the target is taken as `.view(-1)` (a batch of one trains), as in the rest of the family;
  - hist_mask_list may be of any dtype (non-zero = content).
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers.conv import NextItNetLayer


class NextItNet(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(NextItNet, self).__init__(enc_dict, config)

        self.dilations = self.config.get('dilations', None)
        self.one_masked = self.config.get('one_masked', False)
        self.kernel_size = self.config.get('kernel_size', 3)
        self.feat_drop = self.config.get('feat_drop', 0)

        self.nextit_layer = NextItNetLayer(
            self.embedding_dim, self.dilations, self.one_masked, self.kernel_size, feat_drop=self.feat_drop
        )
        self.fc = torch.nn.Linear(self.embedding_dim, self.embedding_dim, bias=False)

        self.reset_parameters()

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        item_seq_len = (data['hist_mask_list'] != 0).sum(dim=1)  # int64, computed once, where the mask lives
        if item_seq.is_cuda:
            # while training one check covers the lookup and the loss (they share the device flag): the loss makes it
            check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
            item_seq_emb = Fh.hist_rows(self.item_emb.weight, item_seq, check_indices=check)
        else:
            item_seq_emb = self.item_emb(item_seq)
        user_emb = self.nextit_layer(item_seq_emb, item_seq_len)
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
