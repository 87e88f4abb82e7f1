"""ComirecDR — drop-in for rec_pangu/models/sequence/comirec.py:67-118 (config key `K` is required).  ComirecSA pools by
attention, not by routing, and is not here yet; it will share the readout.

    interests = CapsuleNetwork(bilinear_type=2)(item_emb(hist), hist_mask_list)        user_emb [B, K, D]
    training:   best[b] = interests[b, argmax_k interests[b, k] . item_emb(target[b])],  loss = full softmax CE of best
On the HIP device: Fh.hist_rows -> Fh.capsule_project (every position its own [K D, D] matrix, one launch for all of them;
the reference's [B, L, K D, D] product is never formed) -> Fh.capsule_route -> Fh.interest_pick -> calculate_loss; the index
check is deferred to the loss while training.  On the CPU the reference's torch formulas.

Deliberate differences, the same three as MIND's (models/sequence/mind.py):
  - the target is taken as `.view(-1)`, as in the rest of the family;
  - the reference's torch.rand(B, D) placeholder for `best_interest_emb` is overwritten in full: the CPU path still draws
    it (the CPU generator's stream and the fixtures match the reference), the device path does not;
  - a history whose second dimension is not max_length raises ValueError on both paths.
"""
from .mind import CapsuleRecallModel


class ComirecDR(CapsuleRecallModel):
    bilinear_type = 2
