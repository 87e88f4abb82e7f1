"""Recall evaluation of the sequence models — counterparts of rec_pangu/utils/evaluate.py, without faiss.

get_recall_predict: the reference L2-normalises the item table and the user embeddings (sklearn.preprocessing.normalize: a
zero row stays zero) and asks a faiss IndexFlatIP for the topN items of every user.  IndexFlatIP is an exact inner-product
search, so the same answer is `topN largest of users @ items.T, in descending order`:
  * HIP device: a chunk of users at a time through the library's Linear forward (hip.linear_fwd: users @ items.T, the score
    buffer capped at SCORE_BUFFER_BYTES), torch.topk(sorted=True) per chunk, the indices copied back once per batch;
  * CPU: numpy.
Fewer than topN items: the tail is -1, as faiss reports a missing neighbour.  The 3-D multi-interest branch keeps the
reference's host-side merge (evaluate.py:70-86).  Users map to LISTS of ints (the reference stores numpy rows, on which its
own evaluate_recall cannot call .index()).

evaluate_recall keeps the reference's arithmetic and its 4-decimal rounding.
"""
import math
from typing import Dict, List

import numpy as np
import torch

SCORE_BUFFER_BYTES = 256 << 20


def _normalize_np(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    norms = np.sqrt(np.einsum('ij,ij->i', x, x))
    norms[norms == 0.0] = 1.0
    return (x / norms[:, None]).astype('float32')


def _normalize_t(x: torch.Tensor) -> torch.Tensor:
    x = x.float()
    norms = torch.sqrt((x * x).sum(dim=1))
    norms = torch.where(norms == 0, torch.ones_like(norms), norms)
    return (x / norms[:, None]).contiguous()


def _pad(idx: np.ndarray, val: np.ndarray, topN: int):
    k = idx.shape[1]
    if k == topN:
        return idx, val
    rows = idx.shape[0]
    return (np.concatenate([idx, np.full((rows, topN - k), -1, dtype=idx.dtype)], axis=1),
            np.concatenate([val, np.full((rows, topN - k), -np.inf, dtype=val.dtype)], axis=1))


def _search_np(users: np.ndarray, items: np.ndarray, topN: int):
    """(indices, scores) of the topN largest inner products of every row of `users`, descending"""
    k = min(topN, items.shape[0])
    rows_per = max(1, SCORE_BUFFER_BYTES // (4 * max(1, items.shape[0])))
    idx_out, val_out = [], []
    for lo in range(0, users.shape[0], rows_per):
        scores = users[lo:lo + rows_per] @ items.T
        idx = np.argsort(-scores, axis=1, kind='stable')[:, :k]
        idx_out.append(idx)
        val_out.append(np.take_along_axis(scores, idx, axis=1))
    if not idx_out:
        return np.zeros((0, topN), dtype=np.int64), np.zeros((0, topN), dtype=np.float32)
    return _pad(np.concatenate(idx_out), np.concatenate(val_out), topN)


def _search_hip(users: torch.Tensor, items: torch.Tensor, topN: int):
    from .. import hip
    k = min(topN, items.shape[0])
    rows_per = max(1, SCORE_BUFFER_BYTES // (4 * max(1, items.shape[0])))
    idx_out, val_out = [], []
    for lo in range(0, users.shape[0], rows_per):
        scores = hip.linear_fwd(users[lo:lo + rows_per], items, None)
        val, idx = torch.topk(scores, k, dim=1, largest=True, sorted=True)
        idx_out.append(idx)
        val_out.append(val)
    if not idx_out:
        return np.zeros((0, topN), dtype=np.int64), np.zeros((0, topN), dtype=np.float32)
    # one copy back per batch
    both = torch.cat([torch.cat(idx_out).double(), torch.cat(val_out).double()], dim=1).cpu().numpy()
    return _pad(both[:, :k].astype(np.int64), both[:, k:].astype(np.float32), topN)


def get_recall_predict(model: torch.nn.Module, test_data, device: torch.device, topN: int = 20) -> dict:
    """{str(user): the topN item ids by inner product of the L2-normalised embeddings, best first} for every user of
    `test_data` (batches with a 'user' entry: a list, or a tensor of ids); model(data, is_training=False)['user_emb'] is
    [B, D], or [B, interests, D] for a multi-interest model (then: every interest's topN merged by score, item 0 and
    repeats dropped, the first topN kept)."""
    item_w = model.output_items().detach()
    on_hip = item_w.is_cuda
    items = _normalize_t(item_w) if on_hip else _normalize_np(item_w.cpu().numpy())
    preds = dict()
    for data in test_data:
        for key in data.keys():
            if key == 'user':
                continue
            data[key] = data[key].to(device)
        model.eval()
        user_embs = model(data, is_training=False)['user_emb'].detach()
        user_list = data['user'] if isinstance(data['user'], list) else data['user'].numpy().tolist()
        interests = user_embs.shape[1] if user_embs.dim() == 3 else 0
        flat = user_embs.reshape(-1, user_embs.shape[-1])
        if on_hip and flat.is_cuda:
            I, S = _search_hip(_normalize_t(flat), items, topN)
        else:
            host_items = items if not on_hip else items.cpu().numpy()
            I, S = _search_np(_normalize_np(flat.cpu().numpy()), host_items, topN)
        if interests == 0:
            for i, user in enumerate(user_list):
                preds[str(user)] = I[i, :].tolist()
            continue
        for i, user in enumerate(user_list):
            rows = slice(i * interests, (i + 1) * interests)
            cand = list(zip(np.reshape(I[rows], -1).tolist(), np.reshape(S[rows], -1).tolist()))
            cand.sort(key=lambda x: x[1], reverse=True)
            chosen = []
            for item, _ in cand:
                if item not in chosen and item != 0:
                    chosen.append(item)
                    if len(chosen) >= topN:
                        break
            preds[str(user)] = chosen
    return preds


def evaluate_recall(preds: Dict[str, List[int]], test_gd: Dict[str, List[int]], topN: int = 50) -> Dict[str, float]:
    """recall@N, ndcg@N and hitrate@N over the users of test_gd (a user without a prediction adds nothing to the sums but
    counts in the divisor), each rounded to 4 decimals.  Per user: recall = hits / len(ground truth); dcg adds
    1 / log2(rank + 2) at the rank of every hit inside the first topN predictions, idcg is the dcg of `hits` leading hits."""
    total_recall, total_ndcg, total_hitrate = 0.0, 0.0, 0
    for user, item_list in test_gd.items():
        if user not in preds:
            continue
        top = list(preds[user][:topN])
        hits, dcg = 0, 0.0
        for item_id in item_list:
            if item_id in top:
                hits += 1
                dcg += 1.0 / math.log(top.index(item_id) + 2, 2)
        idcg = 0.0
        for rank in range(hits):
            idcg += 1.0 / math.log(rank + 2, 2)
        total_recall += hits * 1.0 / len(item_list)
        if hits > 0:
            total_ndcg += dcg / idcg
            total_hitrate += 1
    total = len(test_gd)
    return {f'recall@{topN}': round(total_recall / total, 4), f'ndcg@{topN}': round(total_ndcg / total, 4),
            f'hitrate@{topN}': round(total_hitrate * 1.0 / total, 4)}
