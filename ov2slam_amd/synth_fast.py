"""Seeded test images for the whole-image FAST detector (ov2_fast_detect_batch) and its timing script.  numpy only."""
import numpy as np

MOTIF = 12   # side of the corner motif of `motif_image`


def noise_image(w, h, seed):
    """uniform noise: corners are dense, so every tile edge carries suppression comparisons"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def blocks_image(w, h, seed, n_blocks=12):
    """grey rectangles on a flat ground, smoothed by a 3 x 3 box: a few dozen isolated corners"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 96, np.int32)
    for _ in range(n_blocks):
        bw, bh = int(rng.integers(8, max(9, w // 3))), int(rng.integers(8, max(9, h // 3)))
        x, y = int(rng.integers(0, max(1, w - bw))), int(rng.integers(0, max(1, h - bh)))
        img[y:y + bh, x:x + bw] = int(rng.integers(0, 256))
    p = np.pad(img, 1, mode="edge")
    s = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((s + 4) // 9).astype(np.uint8)


def constant_image(w, h, value=128):
    return np.full((h, w), value, np.uint8)


def dots_image(w, h, dots, ground=200, dot=40):
    """dark single-pixel dots (x, y) on a bright ground: each is a corner of response ground - dot - 1 and nothing else is"""
    img = np.full((h, w), ground, np.uint8)
    for x, y in dots:
        img[y, x] = dot
    return img


def motif_image(nx, ny, ground=200, dot=40):
    """nx x ny copies of one 12 x 12 motif with a dark dot in its middle: nx * ny keypoints that share one response"""
    return dots_image(nx * MOTIF, ny * MOTIF, [(i * MOTIF + MOTIF // 2, j * MOTIF + MOTIF // 2) for j in range(ny) for i in range(nx)],
                      ground, dot)


def noise_blocks_image(w, h, seed, amplitude=24):
    """blocks with mild noise on top (the timing script's image): textured, with strong and weak corners"""
    rng = np.random.default_rng(seed)
    img = blocks_image(w, h, seed, n_blocks=40).astype(np.int32) + rng.integers(-amplitude, amplitude + 1, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def mask_points(w, h, n, seed):
    """n sub-pixel points inside the image"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1).astype(np.float32)
