"""CPU: batching.ragged_chunks, the pure chunking of attack_many_ragged."""
import random

import pytest

import batching


def _cost(k):
    return k[0] + k[1]


@pytest.mark.parametrize("n,max_batch", [(0, 4), (1, 1), (5, 5), (12, 5), (257, 256), (40, 1)])
def test_every_index_once_and_chunk_size(n, max_batch):
    rnd = random.Random(n * 31 + max_batch)
    keys = [(rnd.randint(33, 600), rnd.randint(17, 600)) for _ in range(n)]
    chunks = batching.ragged_chunks(keys, max_batch)
    flat = [i for c in chunks for i in c]
    assert sorted(flat) == list(range(n))
    assert all(1 <= len(c) <= max_batch for c in chunks)
    assert len(chunks) == (n + max_batch - 1) // max_batch
    # longest first: the costs along the chunks, and so the chunks' own, never increase
    costs = [_cost(keys[i]) for i in flat]
    assert costs == sorted(costs, reverse=True)
    sums = [sum(_cost(keys[i]) for i in c) for c in chunks if len(c) == max_batch]
    assert sums == sorted(sums, reverse=True)


def test_ties_keep_input_order():
    keys = [(100, 50), (70, 80), (300, 0), (50, 100), (150, 0), (10, 10)]
    assert batching.ragged_chunks(keys, 4) == [[2, 0, 1, 3], [4, 5]]
    # the emb kind (T_src = 0) is attack_many(ragged=True)'s order: by -T, then input order
    keys = [(64, 0), (300, 0), (128, 0), (300, 0), (64, 0)]
    assert batching.ragged_chunks(keys, 2) == [[1, 3], [2, 0], [4]]


def test_max_batch_must_be_positive():
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_batch"):
            batching.ragged_chunks([(100, 100)], bad)
