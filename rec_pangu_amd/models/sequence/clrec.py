"""CLRec — drop-in for rec_pangu/models/sequence/clrec.py (config key and default as there: temp 0.1).

    user_emb = BERT4RecEncoder(item_emb(hist), len)  (2 layers, 2 heads),  len_b = sum(hist_mask_list[b])
    loss = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
           + ContraLoss(temp)(normalize(user_emb), normalize(item_emb(target)))
where ContraLoss is the in-batch softmax of every user row against every target row of the batch, its own target the
positive.  On the HIP device: Fh.hist_rows -> the encoder (per layer one stacked Q | K | V GEMM and one key-padding
attention launch each way; the final layer runs for the one row per sample that is read) -> the family's fused loss head,
Fh.l2_normalize and Fh.contrastive_loss (csrc/contrast.hip: no [B, B] tensor in either direction).  On the CPU the
reference's torch formulas.

Deliberate differences: the target is taken as `.view(-1)` (a batch of one trains), as in the rest of the family;
hist_mask_list may be of any dtype (non-zero counts); the attention subtracts each row's own maximum where the reference
subtracts the batch's (layers/sequence.py); 'user_emb' is returned while training too.
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers import BERT4RecEncoder


class CLRec(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(CLRec, self).__init__(enc_dict, config)

        self.temp = self.config.get("temp", 0.1)
        self.encoder = BERT4RecEncoder(self.embedding_dim, self.max_length, num_layers=2, num_heads=2)

        self.reset_parameters()

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        item_seq_length = torch.sum(data['hist_mask_list'] != 0, dim=1)
        on_hip = item_seq.is_cuda
        # while training one check covers the lookups and the loss (they share the device flag): the loss makes it
        check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
        seq_emb = Fh.hist_rows(self.item_emb.weight, item_seq, check_indices=check) if on_hip else self.item_emb(item_seq)
        user_emb = self.encoder(seq_emb, item_seq_length)
        if not is_training:
            return {'user_emb': user_emb}
        item = data['target_item'].view(-1)
        if on_hip:
            target_item_emb = Fh.hist_rows(self.item_emb.weight, item.view(-1, 1), check_indices="deferred").squeeze(1)
        else:
            target_item_emb = self.item_emb(item)
        own = torch.arange(item.shape[0], device=item.device)
        loss = self.calculate_loss(user_emb, item)
        loss = loss + Fh.contrastive_loss(Fh.l2_normalize(user_emb), Fh.l2_normalize(target_item_emb), own, own, self.temp)
        return {'user_emb': user_emb, 'loss': loss}
