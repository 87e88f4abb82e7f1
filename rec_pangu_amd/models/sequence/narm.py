"""NARM — drop-in for rec_pangu/models/sequence/narm.py.

    gru_out = GRU(emb_dropout(item_emb(hist)))            (n_layers, hidden_size, no biases, ALL L positions, padding included)
    ht      = gru_out[b, len_b - 1],  len = sum(mask)
    alpha   = v_t((hist > 0) * sigmoid(a_1(gru_out) + a_2(ht)))          (the mask is the id's, not hist_mask_list)
    user_emb = b(ct_dropout(cat[sum_l alpha * gru_out, ht]))
On the HIP device: one recurrence launch per layer and direction (Fh.gru_encode; the rows are gathered inside the first layer's
kernel unless emb_dropout is active, which needs them as a tensor), a_1 / a_2 / b on the library's Linear, the readout in
between as one launch each way (Fh.narm_attention), dropouts on the library's kernel.  On the CPU the reference's formulas.

Deliberate differences: the target is taken as `.view(-1)`; a row without history gives ht = 0 on the HIP device (the CPU
path fails on the gather index -1 like the reference).
"""
from typing import Dict

import torch
from torch import nn

from ... import functional as Fh
from ..base_model import SequenceBaseModel


class NARM(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(NARM, self).__init__(enc_dict, config)

        self.n_layers = self.config.get('n_layers', 2)
        self.dropout_probs = self.config.get('dropout_probs', [0.1, 0.1])
        self.hidden_size = self.config.get('hidden_size', 32)

        self.emb_dropout = nn.Dropout(self.dropout_probs[0])
        self.gru = nn.GRU(self.embedding_dim, self.hidden_size, self.n_layers, bias=False, batch_first=True)
        self.a_1 = nn.Linear(self.hidden_size, self.hidden_size, bias=False)
        self.a_2 = nn.Linear(self.hidden_size, self.hidden_size, bias=False)
        self.v_t = nn.Linear(self.hidden_size, 1, bias=False)
        self.ct_dropout = nn.Dropout(self.dropout_probs[1])
        self.b = nn.Linear(2 * self.hidden_size, self.embedding_dim, bias=False)

        self.reset_parameters()

    def _forward_hip(self, item_seq, item_seq_len, is_training):
        check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
        B, L = item_seq.shape
        steps = torch.full((B,), L, dtype=torch.int32, device=item_seq.device)
        last = (item_seq_len - 1).to(torch.int32)
        if self.training and self.emb_dropout.p > 0:
            x = Fh.dropout(Fh.hist_rows(self.item_emb.weight, item_seq, check_indices=check), self.emb_dropout.p)
            gru_out, ht = Fh.gru_encode(self.gru, steps, last, x=x, packed=False)
        else:
            gru_out, ht = Fh.gru_encode(self.gru, steps, last, ids=item_seq, item_weight=self.item_emb.weight, packed=False,
                                        check_indices=check)
        q1 = Fh.linear_act(gru_out, self.a_1.weight)
        q2 = Fh.linear_act(ht, self.a_2.weight)
        c_t = Fh.narm_attention(q1, q2, self.v_t.weight, item_seq, gru_out, ht)
        if self.training and self.ct_dropout.p > 0:
            c_t = Fh.dropout(c_t, self.ct_dropout.p)
        return Fh.linear_act(c_t, self.b.weight)

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        item_seq_len = torch.sum(data['hist_mask_list'], dim=-1)
        if item_seq.is_cuda:
            user_emb = self._forward_hip(item_seq, item_seq_len, is_training)
        else:
            gru_out, _ = self.gru(self.emb_dropout(self.item_emb(item_seq)))
            ht = self.gather_indexes(gru_out, (item_seq_len - 1).to(torch.int64))
            q1 = self.a_1(gru_out)
            q2 = self.a_2(ht)
            c_t = Fh.narm_attention(q1, q2, self.v_t.weight, item_seq, gru_out, ht)
            user_emb = self.b(self.ct_dropout(c_t))
        if is_training:
            target_item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, target_item)}
        return {'user_emb': user_emb}
