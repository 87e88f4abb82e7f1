"""STAMP — drop-in for rec_pangu/models/sequence/stamp.py (config key and default as there: feat_drop 0).

    lens = sum(hist_mask_list),  valid = (position < lens),  x = feat_drop(item_emb(hist))
    m_s = sum_l valid x_l / lens,  x_t = x[lens - 1]
    alpha_l = valid attn_e(sigmoid(attn_i(x_l) + attn_t(x_t) + attn_s(m_s))),  m_a = sum_l alpha_l x_l
    user_emb = fc_a(m_a) * fc_t(x_t),  loss = full softmax CE
On the HIP device: Fh.hist_rows (+ Fh.dropout while training with feat_drop > 0) -> m_s from Fh.hist_mean over the table,
rescaled from 1 / L to 1 / lens (from the dropped rows through Fh.seq_pool when there is dropout) -> x_t by Fh.seq_take ->
attn_t / attn_s on the library's Linear -> attn_i, attn_e, the mask and the pooling as ONE Fh.attention_pool node
(csrc/attn_pool.hip) -> fc_a / fc_t -> the family's fused loss head; the index check is deferred to the
loss while training.  On the CPU the reference's formulas.

Deliberate differences:
  - the target is taken as `.view(-1)` (a batch of one trains), as in the rest of the family;
  - a row without history (lens = 0): the reference divides by zero and gives NaN; here m_s = x_t = 0, hence
    user_emb = fc_a.bias * fc_t.bias, and no gradient reaches the encoder for that row, on both paths.
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers.sequence import STAMPLayer


class STAMP(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(STAMP, self).__init__(enc_dict, config)

        self.feat_drop = self.config.get('feat_drop', 0)

        self.stamp_layer = STAMPLayer(self.embedding_dim, feat_drop=self.feat_drop)
        self.reset_parameters()

    def _forward_hip(self, item_seq, item_seq_len, is_training):
        # while training one check covers the lookups and the loss (they share the device flag): the loss makes it
        check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
        L = item_seq.shape[1]
        rows = Fh.hist_rows(self.item_emb.weight, item_seq, check_indices=check)
        if self.training and self.feat_drop > 0:
            return self.stamp_layer(rows, item_seq_len)  # (the mean is over the dropped rows)
        valid = torch.arange(L, device=item_seq.device).unsqueeze(0) < item_seq_len.unsqueeze(-1)
        scale = torch.where(item_seq_len > 0, L / item_seq_len.clamp(min=1).to(torch.float32),
                            torch.zeros((), dtype=torch.float32, device=item_seq.device))
        m_s = Fh.hist_mean(self.item_emb.weight, item_seq, valid, check_indices=check) * scale.unsqueeze(-1)
        return self.stamp_layer(rows, item_seq_len, m_s=m_s)

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        item_seq_len = torch.sum(data['hist_mask_list'], dim=1)
        if item_seq.is_cuda:
            user_emb = self._forward_hip(item_seq, item_seq_len, is_training)
        else:
            user_emb = self.stamp_layer(self.item_emb(item_seq), item_seq_len)
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
