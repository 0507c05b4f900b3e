"""Checker of ov2_knn2_hamming_batch (numpy only): cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, 2) as the header
restates it -- Hamming distances from a byte popcount table, the two neighbours of a query = the first two train rows in a
stable sort on (distance, row); a neighbour that does not exist is idx = -1, dist = -1."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(query, train):
    """(n_query, n_train) int32 Hamming distances of 32-byte rows"""
    q = np.asarray(query, np.uint8).reshape(-1, 32)
    t = np.asarray(train, np.uint8).reshape(-1, 32)
    d = np.zeros((len(q), len(t)), np.int32)
    for k in range(32):   # one byte column at a time keeps the intermediate small
        d += POPCOUNT[q[:, k, None] ^ t[None, :, k]]
    return d


def knn2(query, train):
    """(idx, dist), each (n_query, 2) int32"""
    d = distances(query, train)
    nq, nt = d.shape
    idx, dist = np.full((nq, 2), -1, np.int32), np.full((nq, 2), -1, np.int32)
    if nt:
        order = np.argsort(d, axis=1, kind="stable")[:, :2]   # stable: the lower row first among equal distances
        k = order.shape[1]
        idx[:, :k] = order
        dist[:, :k] = np.take_along_axis(d, order, axis=1)
    return idx, dist


def knn2_batch(queries, trains):
    return [knn2(q, t) for q, t in zip(queries, trains)]
