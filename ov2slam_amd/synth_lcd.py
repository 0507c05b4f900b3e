"""Seeded keyframe streams for the loop detector: per keyframe an (n, 32) uint8 array of BRIEF-like descriptors.

Each keyframe keeps roughly half of the previous keyframe's descriptors with 2 - 12 bits flipped (tracked map points whose
descriptor was refreshed) and fills up with new random ones.  With a revisit, keyframe revisit_from + j takes half of its
descriptors from keyframe revisit_to + j instead (the planted loop), a quarter from its predecessor, and the rest new."""
import numpy as np


def _flip(rng, row):
    r = row.copy()
    for bit in rng.choice(256, size=int(rng.integers(2, 13)), replace=False):
        r[bit // 8] ^= np.uint8(1 << (bit % 8))
    return r


def _take(rng, rows, k):
    pick = rng.choice(len(rows), size=min(k, len(rows)), replace=False)
    return [_flip(rng, rows[i]) for i in np.sort(pick)]


def stream(seed, n_kf=40, revisit_from=30, revisit_to=8, empty=()):
    """list of n_kf descriptor arrays; revisit_from = None: no planted loop; keyframes listed in `empty` offer no descriptors
    (their successor continues from the last keyframe that had some)"""
    rng = np.random.default_rng(seed)
    out, last = [], None
    for k in range(n_kf):
        n = int(rng.integers(48, 65))
        if k in empty:
            out.append(np.zeros((0, 32), np.uint8))
            continue
        rows = []
        if revisit_from is not None and k >= revisit_from and len(out[revisit_to + k - revisit_from]):
            rows += _take(rng, out[revisit_to + k - revisit_from], n // 2)
            if last is not None:
                rows += _take(rng, last, n // 4)
        elif last is not None:
            rows += _take(rng, last, n // 2)
        while len(rows) < n:
            rows.append(rng.integers(0, 256, 32, dtype=np.uint8))
        d = np.stack(rows)[rng.permutation(len(rows))]
        out.append(d)
        last = d
    return out


def planted(n_kf=40, revisit_from=30, revisit_to=8):
    """{revisit keyframe: planted keyframe}"""
    return {} if revisit_from is None else {k: revisit_to + k - revisit_from for k in range(revisit_from, n_kf)}
