"""ComirecSA and ComirecDR — drop-ins for rec_pangu/models/sequence/comirec.py:12-64 and :67-118 (config key `K` is required).

ComirecSA:
    interests = MultiInterestSelfAttention(D, K)(item_emb(hist), hist_mask_list)        user_emb [B, K, D]
              = softmax_l(tanh(x W1) W2, masked positions at -1e9)^T x
    training:   the hard readout and the loss below
On the HIP device: Fh.hist_rows -> multi_interest_sa as ONE Fh.attention_pool node (csrc/attn_pool.hip; the
hidden tensor [B, L, 4 D] exists on neither side) -> Fh.interest_pick -> calculate_loss.  A row without history pools
uniformly over all L rows, as the reference's; its masked scores are constants, so it passes no gradient to W1 / W2.

ComirecDR:
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
from .mind import CapsuleRecallModel, MultiInterestRecallModel
from ..layers.multi_interest import MultiInterestSelfAttention


class ComirecSA(MultiInterestRecallModel):
    def __init__(self, enc_dict, config):
        super(ComirecSA, self).__init__(enc_dict, config)

        self.multi_interest_sa = MultiInterestSelfAttention(embedding_dim=self.embedding_dim,
                                                            num_attention_heads=self.config['K'])
        self.reset_parameters()

    def interests(self, seq_emb, mask):
        return self.multi_interest_sa(seq_emb, mask.unsqueeze(-1).float())


class ComirecDR(CapsuleRecallModel):
    bilinear_type = 2
