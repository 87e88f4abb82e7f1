"""MIND — drop-in for rec_pangu/models/sequence/mind.py (config key `K`, the number of interests, is required).

    interests = CapsuleNetwork(bilinear_type=0)(item_emb(hist), hist_mask_list)        user_emb [B, K, D]
    training:   best[b] = interests[b, argmax_k interests[b, k] . item_emb(target[b])],  loss = full softmax CE of best
On the HIP device: Fh.hist_rows -> the library's Linear -> Fh.capsule_route (one launch each way, the rows read by all K
interests with stride 0) -> Fh.interest_pick (one launch instead of the reference's Python loop over the batch) ->
calculate_loss; the index check is deferred to the loss while training.  On the CPU the reference's torch formulas.

Deliberate differences:
  - the target is taken as `.view(-1)` (a batch of one trains), as in the rest of the family;
  - the reference fills `best_interest_emb` from a torch.rand(B, D) placeholder that is overwritten in full.  The CPU path
    still draws it, so the CPU generator's stream (and the fixtures) match the reference; the device path does not draw it:
    only the position of the CPU generator differs there;
  - a history whose second dimension is not max_length raises ValueError on both paths (the reference mis-reshapes it or
    fails later).
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers.multi_interest import CapsuleNetwork


class MultiInterestRecallModel(SequenceBaseModel):
    """what MIND, ComirecDR and ComirecSA share: K interests [B, K, D] from the history's item rows (`interests`, the
    subclass's encoder) and the hard readout"""

    def interests(self, seq_emb, mask):
        raise NotImplementedError

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        mask = data['hist_mask_list']
        if item_seq.shape[1] != self.max_length:
            raise ValueError(f"{type(self).__name__}: hist_item_list has {item_seq.shape[1]} positions, max_length is "
                             f"{self.max_length}")
        on_hip = item_seq.is_cuda
        # while training one check covers every launch (they share the device flag): the loss makes it
        check = "deferred" if (is_training or self.check_indices != "sync") else "sync"
        seq_emb = Fh.hist_rows(self.item_emb.weight, item_seq, check_indices=check)  # Batch,Seq,Emb
        multi_interest_emb = self.interests(seq_emb, mask)  # Batch,K,Emb
        if not is_training:
            return {'user_emb': multi_interest_emb}
        item = data['target_item'].view(-1)
        if not on_hip:
            torch.rand(multi_interest_emb.shape[0], multi_interest_emb.shape[2])  # (the reference's placeholder draw)
        best_interest_emb = Fh.interest_pick(multi_interest_emb, self.item_emb.weight, item, check_indices="deferred")
        loss = self.calculate_loss(best_interest_emb, item)
        return {'user_emb': multi_interest_emb, 'loss': loss}


class CapsuleRecallModel(MultiInterestRecallModel):
    """MIND and ComirecDR: a CapsuleNetwork over the rows"""
    bilinear_type = 0

    def __init__(self, enc_dict, config):
        super(CapsuleRecallModel, self).__init__(enc_dict, config)

        self.capsule = CapsuleNetwork(self.embedding_dim, self.max_length, bilinear_type=self.bilinear_type,
                                      interest_num=self.config['K'])
        self.reset_parameters()

    def interests(self, seq_emb, mask):
        return self.capsule(seq_emb, mask, self.device)


class MIND(CapsuleRecallModel):
    bilinear_type = 0
