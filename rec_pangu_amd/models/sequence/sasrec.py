"""SASRec — drop-in for rec_pangu/models/sequence/sasrec.py (config keys and defaults as there: n_layers 2, n_heads 4,
inner_size 32, hidden_dropout_prob / attn_dropout_prob 0.1, hidden_act 'gelu', layer_norm_eps 0.001; hidden_size is read and
ignored, the encoder's width is embedding_dim).

    user_emb = TransformerEncoder(item_emb(hist), causal + padding mask)[-1][b, len_b - 1],  len_b = sum(hist_mask_list[b])
    loss = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
On the HIP device: Fh.hist_rows -> TransformerEncoder.encode_last (per layer one stacked Q | K | V GEMM and one fused
attention launch each way, no [B, heads, L, L] tensor; the final layer runs for the one row per sample that is read) -> the
family's fused loss head.  On the CPU the reference's torch formulas (get_attention_mask, the encoder, gather_indexes).

Deliberate differences:
  - the target is taken as `.view(-1)` (a batch of one trains), as in the rest of the family;
  - hist_mask_list may be of any dtype (non-zero = content);
  - a row without history gives a zero user_emb on the HIP device and takes no gradient through the encoder: it never reaches a device-side index check (the CPU path raises inside gather like the reference).
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers.transformer import TransformerEncoder


class SASRec(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(SASRec, self).__init__(enc_dict, config)

        self.n_layers = config.get('n_layers', 2)
        self.n_heads = config.get('n_heads', 4)
        self.hidden_size = config.get('hidden_size', 64)  # same as embedding_size
        self.inner_size = config.get('inner_size', 32)  # the dimensionality in feed-forward layer
        self.hidden_dropout_prob = config.get('hidden_dropout_prob', 0.1)
        self.attn_dropout_prob = config.get('attn_dropout_prob', 0.1)
        self.hidden_act = config.get('hidden_act', 'gelu')
        self.layer_norm_eps = config.get('layer_norm_eps', 0.001)

        self.self_attention = TransformerEncoder(
            n_layers=self.n_layers,
            n_heads=self.n_heads,
            hidden_size=self.embedding_dim,
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
        if item_seq.is_cuda:
            # while training one check covers the lookup and the loss (they share the device flag): the loss makes it
            check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
            item_seq_emb = Fh.hist_rows(self.item_emb.weight, item_seq, check_indices=check)
            user_emb = self.self_attention.encode_last(item_seq_emb, mask)
        else:
            item_seq_len = torch.sum(mask, dim=-1).long()
            item_seq_emb = self.item_emb(item_seq)
            attention_mask = self.get_attention_mask(mask)
            output = self.self_attention(item_seq_emb, attention_mask, output_all_encoded_layers=True)[-1]
            user_emb = self.gather_indexes(output, item_seq_len - 1)
        if is_training:
            item = data['target_item'].view(-1)
            return {'user_emb': user_emb, 'loss': self.calculate_loss(user_emb, item)}
        return {'user_emb': user_emb}
