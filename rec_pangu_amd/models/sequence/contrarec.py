"""ContraRec — drop-in for rec_pangu/models/sequence/contrarec.py (config keys and defaults as there: gamma 1, beta_a and
beta_b 3, ctc_temp and ccc_temp 0.2, encoder_name 'BERT4Rec').

    user_emb = encoder(item_emb(hist), len),  len_b = sum(hist_mask_list[b])
    loss = CrossEntropyLoss()(user_emb @ item_emb.weight.T, target)
           + gamma * ContraLoss(ccc_temp)(normalize(cat(encoder(aug1), encoder(aug2))), cat(target, target))
with aug1, aug2 two random augmentations of the history (DataAugmenter) and ContraLoss the supervised in-batch contrastive
loss over the 2 B views: the other view and every view of a row with the same target are positives, the view itself is left
out.  Encoders: 'BERT4Rec' (layers.BERT4RecEncoder, 2 layers, 2 heads), 'GRU4Rec' (layers.GRU4RecEncoder, hidden 128);
'Caser' raises NotImplementedError (its conv stack is not ported), any other name ValueError.

The history and its two augmentations are encoded as ONE pass over 3 B rows: the weights are shared and the encoders have
no dropout and no batch statistic, so this is the same function as the reference's three passes.  On the HIP device:
Fh.hist_rows (the mask token's row broadcast beside it), the encoder's kernels, the family's fused loss head, Fh.l2_normalize and
Fh.contrastive_loss (csrc/contrast.hip: no [2 B, 2 B] tensor in either direction; the reference materialises it about
seven times).  On the CPU the reference's torch formulas.

Deliberate differences: the target is taken as `.view(-1)`; hist_mask_list may be of any dtype (non-zero counts); the
attention subtracts each row's own maximum (layers/sequence.py); DataAugmenter is vectorised and draws another random stream
(see there); 'user_emb' is returned while training too.
"""
from typing import Dict

import torch

from ... import functional as Fh
from ..base_model import SequenceBaseModel
from ..layers import BERT4RecEncoder, GRU4RecEncoder


class DataAugmenter:
    """The reference's two sequence augmentations (contrarec.py:147-180), per row a fair coin between them:
      mask     count = int(L * ratio) positions, chosen uniformly over all L, are set to num_items;
      reorder  a window of count positions at a uniform start in [0, L - count] is permuted uniformly; the rest stays;
    ratio ~ Beta(beta_a, beta_b) per row.  Both act on the whole padded row, pads included, as the reference's do.

    The reference loops over the rows in Python with an `.item()` per draw (two host syncs per row).  Here every draw is one
    torch op over the batch on the tensor's device, no sync.  The random STREAM is therefore not the reference's; the
    distribution of each row's result is."""

    def __init__(self, beta_a, beta_b, num_items):
        self.beta_a = beta_a
        self.beta_b = beta_b
        self.num_items = num_items

    def augment(self, seqs: torch.Tensor, return_plan: bool = False):
        """seqs int64 [B, L] -> the augmented copy; with return_plan also (is_mask bool [B], count int64 [B], start int64 [B])
        (start is drawn for every row and read by the reorder rows only)"""
        B, L = seqs.shape
        dev = seqs.device
        is_mask = torch.rand(B, device=dev) > 0.5
        beta = torch.distributions.beta.Beta(torch.tensor(float(self.beta_a), device=dev),
                                             torch.tensor(float(self.beta_b), device=dev))
        count = (L * beta.sample((B,))).long().clamp_(0, L)
        pos = torch.arange(L, device=dev).unsqueeze(0)
        # mask: the `count` smallest of L uniform keys mark a uniform subset of that size
        rank = torch.rand(B, L, device=dev).argsort(dim=1).argsort(dim=1)
        masked = torch.where(rank < count.unsqueeze(1), torch.full_like(seqs, self.num_items), seqs)
        # reorder: inside the window the sort key is start + U[0, 1), outside it the position itself
        start = (torch.rand(B, device=dev, dtype=torch.float64) * (L - count + 1)).long().clamp_(max=L).minimum(L - count)
        inside = (pos >= start.unsqueeze(1)) & (pos < (start + count).unsqueeze(1))
        key = torch.where(inside, start.unsqueeze(1) + torch.rand(B, L, device=dev, dtype=torch.float64), pos.double())
        reordered = seqs.gather(1, key.argsort(dim=1, stable=True))
        out = torch.where(is_mask.unsqueeze(1), masked, reordered)
        if return_plan:
            return out, (is_mask, count, start)
        return out


class ContraRec(SequenceBaseModel):
    def __init__(self, enc_dict, config):
        super(ContraRec, self).__init__(enc_dict, config)

        self.gamma = self.config.get("gamma", 1)
        self.beta_a = self.config.get("beta_a", 3)
        self.beta_b = self.config.get("beta_b", 3)
        self.ctc_temp = self.config.get("ctc_temp", 0.2)
        self.ccc_temp = self.config.get("ccc_temp", 0.2)
        self.encoder_name = self.config.get("encoder_name", "BERT4Rec")
        self.encoder = self.init_encoder(self.encoder_name)
        self.data_augmenter = DataAugmenter(beta_a=self.beta_a,
                                            beta_b=self.beta_b,
                                            num_items=self.enc_dict[self.config['item_col']]['vocab_size'] - 1)

        self.reset_parameters()

    def init_encoder(self, encoder_name):
        if encoder_name == 'GRU4Rec':
            encoder = GRU4RecEncoder(self.embedding_dim, hidden_size=128)
        elif encoder_name == 'Caser':
            raise NotImplementedError("ContraRec: encoder_name 'Caser' needs CaserEncoder, whose conv stack is not ported; "
                                      "use 'BERT4Rec' or 'GRU4Rec'")
        elif encoder_name == 'BERT4Rec':
            encoder = BERT4RecEncoder(self.embedding_dim, self.max_length, num_layers=2, num_heads=2)
        else:
            raise ValueError('Invalid sequence encoder.')
        return encoder

    def encode(self, item_seq: torch.Tensor, lengths: torch.Tensor, check: str = "deferred") -> torch.Tensor:
        """item ids [N, L], lengths [N] -> [N, D] through the configured encoder"""
        if not item_seq.is_cuda:
            return self.encoder(self.item_emb(item_seq), lengths)
        # The mask augmentation writes ONE id, num_items, into an eighth of all positions, and the lookup's backward has one
        # writer per table row walk that row's occurrences in order (25 ms at B = 4096, L = 20).  That id's row is therefore
        # broadcast and selected, and the lookup sees the padding id in its place.
        token = self.data_augmenter.num_items
        is_token = item_seq == token
        rows = Fh.hist_rows(self.item_emb.weight, item_seq.masked_fill(is_token, 0), check_indices=check)
        rows = torch.where(is_token.unsqueeze(-1), self.item_emb.weight[token].view(1, 1, -1), rows)
        return self.encoder(rows, lengths)

    def forward(self, data: Dict[str, torch.Tensor], is_training: bool = True):
        item_seq = data['hist_item_list']
        item_seq_length = torch.sum(data['hist_mask_list'] != 0, dim=1)
        if not is_training:
            return {'user_emb': self.encode(item_seq, item_seq_length, "deferred" if self.check_indices != "sync" else "sync")}
        item = data['target_item'].view(-1)
        B = item_seq.shape[0]
        aug_seq1 = self.data_augmenter.augment(item_seq)
        aug_seq2 = self.data_augmenter.augment(item_seq)
        # one pass over the 3 B rows (the loss's index check covers the lookups: they share the device flag)
        emb = self.encode(torch.cat([item_seq, aug_seq1, aug_seq2], dim=0), item_seq_length.repeat(3))
        user_emb = emb[:B]
        features = Fh.l2_normalize(emb[B:])  # cat(view 1, view 2): the reference's cat(unbind(features, dim=1))
        ccc = Fh.contrastive_loss(features, None, torch.cat([item, item]), None, self.ccc_temp, exclude_self=True,
                                  scale=self.ccc_temp)
        loss = self.calculate_loss(user_emb, item) + self.gamma * ccc
        return {'user_emb': user_emb, 'loss': loss}
