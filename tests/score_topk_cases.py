"""What the score top-n tests share, computed outside the code under test."""

import numpy as np


def expected_topk(matrix, top_n):
    """float [B, P] -> (ids int32, scores float32) [B, top_n]: float64
    scores ordered by (-score, id), cut to > 0, padded with (-1, 0.0)."""
    m = np.asarray(matrix, dtype=np.float64)
    B, P = m.shape
    ids = np.full((B, top_n), -1, dtype=np.int32)
    scores = np.zeros((B, top_n), dtype=np.float32)
    for b in range(B):
        order = np.lexsort((np.arange(P), -m[b]))
        order = order[m[b][order] > 0][:top_n]
        ids[b, :len(order)] = order
        scores[b, :len(order)] = m[b][order]
    return ids, scores


def tie_matrix(P, seed, rows=6):
    """float32 [rows, P] from {0, 0.5, 1, 1.5}: ties everywhere.  Row 1 is
    all zero, row 2 has at most two positives, the last none that is 0."""
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array([0, 0.5, 1, 1.5], dtype=np.float32),
                   size=(rows, P))
    m[1] = 0
    m[2] = 0
    m[2, [0, P - 1]] = [0.5, 1.5][:len({0, P - 1})]
    m[-1] = np.maximum(m[-1], np.float32(0.5))
    return m
