"""The policy of the sort cache (rec_pangu_amd/models/layers/embedding.py: SortedLookup, _SORT_CACHE, _SORT_PINNED): pure
python over tensor identity and version counters, so it is checked on CPU tensors with hand-made entries."""
import gc
import weakref

import pytest
import torch

from rec_pangu_amd.models.layers import embedding as E

SIG = ((8, 4), "cpu")


@pytest.fixture(autouse=True)
def _empty_caches():
    saved = E._SORT_CACHE[:], E._SORT_PINNED[:]
    del E._SORT_CACHE[:], E._SORT_PINNED[:]
    yield
    E._SORT_CACHE[:], E._SORT_PINNED[:] = saved


def _batch():
    return {"C0": torch.arange(6), "C1": torch.arange(6) % 4}


def _look(X, sig=SIG, pinned=False):
    buf = [torch.zeros(12, dtype=torch.int32) for _ in range(3)]
    return E.SortedLookup(*buf, tuple(X.values()), sig, pinned=pinned)


def test_a_refill_in_place_ends_an_unpinned_match_and_keeps_a_pinned_one():
    X = _batch()
    src = tuple(X.values())
    plain, pinned = _look(X), _look(X, pinned=True)
    E.EmbeddingLayer._cache_sort(plain)
    assert plain.matches(src, SIG) and pinned.matches(src, SIG)
    assert E._find_sort(src, SIG) is plain and E._find_sort(src, SIG, cached=False) is None
    E._SORT_PINNED.append(pinned)
    assert E._find_sort(src, SIG) is pinned  # (pinned entries are asked first)
    # same values in other tensors, another arena signature, fewer tensors: no match
    assert not plain.matches(tuple(t.clone() for t in src), SIG) and not pinned.matches(tuple(t.clone() for t in src), SIG)
    assert not plain.matches(src, ((8, 5), "cpu")) and not pinned.matches(src, ((8, 5), "cpu"))
    assert not plain.matches(src[:1], SIG) and not pinned.matches(src[:1], SIG)
    X["C1"].add_(1)  # the loader refills its buffer in place: the version counter moves
    assert not plain.matches(src, SIG)
    assert pinned.matches(src, SIG)
    assert E._find_sort(src, SIG) is pinned
    del E._SORT_PINNED[:]
    assert E._find_sort(src, SIG) is None


def test_the_unpinned_cache_keeps_the_last_four():
    batches = [_batch() for _ in range(5)]
    looks = [_look(X) for X in batches]
    for look in looks[:4]:
        E.EmbeddingLayer._cache_sort(look)
    assert E._SORT_CACHE == looks[:4]
    E.EmbeddingLayer._cache_sort(looks[4])
    assert E._SORT_CACHE == looks[1:]
    assert E._find_sort(tuple(batches[0].values()), SIG) is None
    assert all(E._find_sort(tuple(X.values()), SIG) is look for X, look in zip(batches[1:], looks[1:]))


def test_unpin_sorts_drops_the_entries_of_one_batch_or_all_and_lets_go_of_their_tensors():
    batches = [_batch() for _ in range(3)]
    looks = [_look(X, pinned=True) for X in batches]
    # a second layer (other arena signature) pinned over the first batch's tensors: an entry of that batch too
    other = _look(batches[0], sig=((9, 9), "cpu"), pinned=True)
    E._SORT_PINNED.extend(looks + [other])
    for look in looks:  # marks and a workspace hang on the entry, nowhere else
        look.smp = tuple(torch.zeros(4, dtype=torch.int32) for _ in range(3))
        look.workspace = torch.zeros(16, dtype=torch.uint8)
    refs = [[weakref.ref(t) for t in (look.keys, look.sk, look.sp, look.workspace) + look.smp] for look in looks]
    E.EmbeddingLayer.unpin_sorts(batches[0])
    assert E._SORT_PINNED == looks[1:]
    del looks, other, look
    gc.collect()
    assert all(r() is None for r in refs[0])
    assert all(r() is not None for rs in refs[1:] for r in rs)
    E.EmbeddingLayer.unpin_sorts()
    assert E._SORT_PINNED == []
    gc.collect()
    assert all(r() is None for rs in refs for r in rs)
    id_ref = weakref.ref(batches[1]["C0"])  # ... and the id tensors themselves are no longer held
    del batches
    gc.collect()
    assert id_ref() is None
