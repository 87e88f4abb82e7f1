"""SequenceDataset / SequenceDatasetV2 / seq_collate — counterparts of rec_pangu/dataset/sequence_dataset.py.

One sample per USER: a window of at most `max_length` items in front of a cut position k, right-padded with id 0 and
masked (`hist_item_list`, `hist_mask_list`, int64 [max_length]), plus what the phase adds:
    SequenceDataset    train: k drawn from [4, len) with the `random` module (one draw per sample), `target_item` [1],
                       the next `next_seq_length` items and their mask; otherwise: k = int(0.8 len) and the user id as
                       a string; get_test_gd(): every item from that cut on
    SequenceDatasetV2  leave-one-out: train k = len - 3, valid k = len - 2, test k = len - 1; get_test_gd(): the one
                       item at the valid / test cut
Samples, dtypes and the enc_dict are the reference's, value for value (tests/golden/sequence_dataset.json).  Like the
reference, encoding writes the encoded columns back into the frame the dataset holds (the caller's frame when no
`time_col` sorts it into a copy first).
"""
import random

import torch
from torch.utils.data import Dataset


def _tensor(values, drop_outer: bool = False):
    # (through float32 like the reference's torch.Tensor(list).long(): ids above 2^24 would round the same way)
    t = torch.tensor(values, dtype=torch.float32)
    return (t.squeeze(0) if drop_outer else t).long()


class SequenceDataset(Dataset):
    def __init__(self, config, df, enc_dict=None, phase='train'):
        self.config = config
        self.df = df
        self.enc_dict = enc_dict
        self.max_length = config['max_length']
        self.user_col = config['user_col']
        self.item_col = config['item_col']
        self.time_col = config.get('time_col', None)
        self.cate_cols = config.get('cate_cols', [])
        self.next_seq_length = config.get('next_seq_length', 10)
        if self.time_col:
            self.df = self.df.sort_values(by=[self.user_col, self.time_col])
        if self.enc_dict is None:
            self.get_enc_dict()
        self.enc_data()
        self.user2item = self._per_user(self.item_col)
        for col in self.cate_cols:
            setattr(self, f'user2{col}', self._per_user(col))
        self.user_list = self.df[self.user_col].unique()
        self.phase = phase

    def _per_user(self, col):
        return self.df.groupby(self.user_col)[col].apply(list).to_dict()

    def _sparse_cols(self):
        return [self.item_col] + self.cate_cols

    def get_enc_dict(self):
        """value (as a string, in sorted order) -> 1, 2, ...; 0 is the padding / unknown id; vocab_size counts it"""
        if self.enc_dict is not None:
            return self.enc_dict
        self.enc_dict = {}
        for f in self._sparse_cols():
            self.df[f] = self.df[f].astype('str')
            values = sorted(self.df[f].unique())
            mapping = {v: i for i, v in enumerate(values, start=1)}
            mapping['vocab_size'] = len(values) + 1
            self.enc_dict[f] = mapping

    def enc_data(self):
        for f in self._sparse_cols():
            table = self.enc_dict[f]
            self.df[f] = self.df[f].astype('str').apply(lambda x: table.get(x, 0))

    # ---- one sample ---------------------------------------------------------------------------------------------------
    def _window(self, seq, k):
        """the max_length entries of seq in front of position k, right-padded with 0"""
        if k >= self.max_length:
            return seq[k - self.max_length: k]
        return seq[:k] + [0] * (self.max_length - k)

    def _history(self, user_id, k):
        n = min(k, self.max_length)
        data = {'hist_item_list': _tensor(self._window(self.user2item[user_id], k)),
                'hist_mask_list': _tensor([1.0] * n + [0.0] * (self.max_length - n))}
        cates = {}
        for col in self.cate_cols:
            window = self._window(getattr(self, f'user2{col}')[user_id], k)
            setattr(self, f'hist_{col}_list', window)
            cates[f'hist_{col}_list'] = _tensor(window, drop_outer=True)
        return data, cates

    def _train_cut(self, item_list):
        return random.choice(range(4, len(item_list)))

    def _eval_cut(self, item_list):
        return int(0.8 * len(item_list))

    def _train_extras(self, item_list, k):
        nxt = item_list[k:k + self.next_seq_length]
        mask = [1] * len(nxt)
        pad = self.next_seq_length - len(nxt)
        return {'next_item_list': _tensor(nxt + [0] * pad, drop_outer=True),
                'next_mask_list': _tensor(mask + [0] * pad, drop_outer=True)}

    def __getitem__(self, index):
        user_id = self.user_list[index]
        item_list = self.user2item[user_id]
        if self.phase == 'train':
            k = self._train_cut(item_list)
            hist, cates = self._history(user_id, k)
            data = dict(hist)
            data['target_item'] = _tensor([item_list[k]])
            data.update(self._train_extras(item_list, k))
        else:
            hist, cates = self._history(user_id, self._eval_cut(item_list))
            data = {'user': str(user_id)}
            data.update(hist)
        data.update(cates)
        return data

    def __len__(self):
        return len(self.user_list)

    def get_test_gd(self):
        self.test_gd = {str(user): items[int(0.8 * len(items)):] for user, items in self.user2item.items()}
        return self.test_gd


class SequenceDatasetV2(SequenceDataset):
    def _train_cut(self, item_list):
        return len(item_list) - 3

    def _eval_cut(self, item_list):
        return len(item_list) - (2 if self.phase == 'valid' else 1)

    def _train_extras(self, item_list, k):
        return {}

    def get_test_gd(self):
        self.test_gd = {str(user): [items[self._eval_cut(items)]] for user, items in self.user2item.items()}
        return self.test_gd


def seq_collate(batch):
    """batch of (hist_item [L], hist_mask [L], item) tuples -> (int64 [n, L], int64 [n, L], list of the items).  The two
    staging buffers are drawn with torch.rand, as in the reference: a run seeded like a reference run stays on its stream."""
    n, L = len(batch), batch[0][0].shape[0]
    hist_item, hist_mask = torch.rand(n, L), torch.rand(n, L)
    for i, sample in enumerate(batch):
        hist_item[i] = sample[0]
        hist_mask[i] = sample[1]
    return hist_item.long(), hist_mask.long(), [sample[2] for sample in batch]
