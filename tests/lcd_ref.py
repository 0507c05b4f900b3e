"""Checker of the loop detector (plain Python / numpy, independent of the C++ and of the kernels).

search2: the exact two nearest live words of every query row by 256-bit Hamming distance, ties to the lower slot -- what
ov2_lcd_search2_batch and the host detector's brute-force back end must return."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(query, rows):
    """(n_query, n_rows) int32 Hamming distances of 32-byte rows"""
    q = np.asarray(query, np.uint8).reshape(-1, 32)
    t = np.asarray(rows, np.uint8).reshape(-1, 32)
    d = np.zeros((len(q), len(t)), np.int32)
    for k in range(32):   # one byte column at a time keeps the intermediate small
        d += POPCOUNT[q[:, k, None] ^ t[None, :, k]]
    return d


def search2(query, rows, dead=None):
    """(idx, dist), each (n_query, 2) int32: slots of the two live rows with the smallest (distance, slot); -1 / -1 where
    fewer live rows exist.  dead: boolean mask over the rows, or None."""
    q = np.asarray(query, np.uint8).reshape(-1, 32)
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    live = np.arange(len(rows)) if dead is None else np.flatnonzero(~np.asarray(dead, bool))
    idx, dist = np.full((len(q), 2), -1, np.int32), np.full((len(q), 2), -1, np.int32)
    if len(live) == 0 or len(q) == 0:
        return idx, dist
    for lo in range(0, len(q), 64):   # blocks of queries keep the distance matrix small for large tables
        d = distances(q[lo:lo + 64], rows[live])
        order = np.argsort(d, axis=1, kind="stable")[:, :2]   # stable: the lower slot first among equal distances
        k = order.shape[1]
        idx[lo:lo + 64, :k] = live[order]
        dist[lo:lo + 64, :k] = np.take_along_axis(d, order, axis=1)
    return idx, dist


# ---- the detector: obindex2::ImageIndex (binary_index.cc) and ibow_lcd::LCDetector (lcdetector.cc, island.h) restated --------
# Departures from the reference, the same five as ov2slam_amd/host/ov2_lcd.hpp: the word search is exact; ties of distance go
# to the lower word id; sorts are descending score with ties by ascending image id / island img_id; a query row with fewer
# than two neighbours is not matched; merge_policy is NONE.

LC_DETECTED, LC_NOT_DETECTED, LC_NOT_ENOUGH_IMAGES, LC_NOT_ENOUGH_ISLANDS = 0, 1, 2, 3
U32 = 0xffffffff


class Params:
    def __init__(self, p=100, nndr=0.8, min_score=0.3, island_size=20, nframes_after_lc=10, purge_descriptors=True, min_feat_apps=2):
        self.p, self.nndr, self.min_score, self.island_size = p, np.float32(nndr), float(min_score), island_size
        self.nframes_after_lc, self.purge_descriptors, self.min_feat_apps = nframes_after_lc, purge_descriptors, min_feat_apps


class ImageIndex:
    def __init__(self, purge_descriptors=True, min_feat_apps=2):
        self.purge_descriptors, self.min_feat_apps = purge_descriptors, min_feat_apps
        self.words = {}            # word id -> (descriptor, [(image_id, kp_ind, dist)]); insertion order = ascending id
        self.ndesc, self.nimages = 0, 0
        self.recently_added = []
        self.added, self.purged = [], []   # of the last addImage

    def _insert(self, desc, item):
        self.words[self.ndesc] = (np.array(desc, np.uint8), [item])
        self.recently_added.append(self.ndesc)
        self.added.append(self.ndesc)
        self.ndesc += 1

    def search(self, descs):
        """per query row the list of up to two (word id, distance), nearest first, ties to the lower word id"""
        ids = np.fromiter(self.words.keys(), np.int64, len(self.words))
        rows = np.stack([w[0] for w in self.words.values()]) if len(ids) else np.zeros((0, 32), np.uint8)
        idx, dist = search2(descs, rows)
        return [[(int(ids[i]), int(d)) for i, d in zip(ri, rd) if i >= 0] for ri, rd in zip(idx, dist)]

    def add_image(self, image_id, descs, matches=None):
        """matches: None (binary_index.cc:48-80) or a list of (query row, word id, distance) (:82-152)"""
        self.added, self.purged = [], []
        descs = np.asarray(descs, np.uint8).reshape(-1, 32)
        if matches is None:
            for i in range(len(descs)):
                self._insert(descs[i], (image_id, i, 0.0))
        else:
            matched = {m[0] for m in matches}
            for i in range(len(descs)):
                if i not in matched:
                    self._insert(descs[i], (image_id, i, 0.0))
            for q, w, d in matches:
                self.words[w][1].append((image_id, q, float(d)))
        if self.purge_descriptors:
            self._purge(image_id)
        self.nimages += 1

    def _purge(self, curr_img):
        keep = []
        for w in self.recently_added:
            items = self.words[w][1]
            if ((curr_img - items[0][0]) & U32) > 1:
                if len(items) < self.min_feat_apps:
                    del self.words[w]
                    self.purged.append(w)
            else:
                keep.append(w)
        self.recently_added = keep

    def search_images(self, nrows, matches):
        """scores of images 0 .. nimages - 1 (binary_index.cc:154-203), unsorted"""
        import math
        score = [0.0] * self.nimages
        nwi = {}
        for _, w, _ in matches:
            nwi[w] = nwi.get(w, 0) + 1
        for _, w, _ in matches:
            items = self.words[w][1]
            tf = float(nwi[w]) / nrows
            idf = math.log(float(self.nimages) / len({it[0] for it in items}))
            tfidf = tf * idf
            for it in items:
                score[it[0]] += tfidf
        return score


class Island:
    def __init__(self, img_id, score, mn, mx):
        self.img_id, self.score, self.min_img_id, self.max_img_id = img_id, score, mn, mx

    def fits(self, i):
        return self.min_img_id <= i <= self.max_img_id

    def overlaps(self, o):
        a1, a2, b1, b2 = self.min_img_id, self.max_img_id, o.min_img_id, o.max_img_id
        return (b1 <= a1 <= b2) or (a1 <= b1 <= a2)

    def adjust_limits(self, i, mn, mx):
        if i > self.max_img_id:
            if mn <= self.max_img_id:
                mn = (self.max_img_id + 1) & U32
        elif mx >= self.min_img_id:
            mx = (self.min_img_id - 1) & U32
        return mn, mx

    def tuple(self):
        return (self.img_id, self.min_img_id, self.max_img_id, self.score)


def build_islands(image_matches, island_size):
    """image_matches: [(image id, score)] in the order filterCandidates leaves them.  lcdetector.cc:206-252"""
    off = island_size // 2
    islands = []
    for img, sc in image_matches:
        mn, mx = max(img - off, 0), img + off
        for isl in islands:
            if isl.fits(img):
                isl.score += sc
                break
            mn, mx = isl.adjust_limits(img, mn, mx)
        else:
            islands.append(Island(img, sc, mn, mx))
    for isl in islands:
        isl.score = isl.score / (((isl.max_img_id - isl.min_img_id + 1)) & U32)
    islands.sort(key=lambda s: (-s.score, s.img_id))
    return islands


def _min_gap(values):
    """smallest non-zero gap between neighbours of a sorted list (exact ties are decided by the tie rule, not by a double)"""
    g = [abs(a - b) for a, b in zip(values, values[1:]) if a != b]
    return min(g) if g else float("inf")


class LCDetector:
    def __init__(self, params):
        self.P = params
        self.index = ImageIndex(params.purge_descriptors, params.min_feat_apps)
        self.last_island = Island(U32, 0.0, U32, U32)   # Island(-1, 0.0, -1, -1) in unsigned
        self.last_query_id = 1                          # LCDetectorResult() leaves query_id = 1
        self.queue, self.prev_descs = [], []
        self.trace = []

    def filter_matches(self, feats):
        out = []
        for q, m in enumerate(feats):
            if len(m) < 2:
                continue
            if np.float32(m[0][1]) <= np.float32(m[1][1]) * self.P.nndr:   # float, lcdetector.cc:177
                out.append((q, m[0][0], m[0][1]))
        return out

    def _add_image(self, image_id, descs):
        if self.index.nimages == 0:
            self.index.add_image(image_id, descs)
            return []
        m = self.filter_matches(self.index.search(descs))
        self.index.add_image(image_id, descs, m)
        return m

    def process(self, image_id, descs):
        """returns (status, train_id); appends a dict to self.trace"""
        descs = np.asarray(descs, np.uint8).reshape(-1, 32)
        t = dict(query_id=image_id, status=None, train_id=0, add_matches=[], added=[], purged=[], matches=[], scores=[], islands=[],
                 margin=float("inf"), nwords=len(self.index.words))
        self.trace.append(t)
        assert image_id == len(self.prev_descs)
        self.prev_descs.append(descs)
        self.queue.append(image_id)
        if len(self.queue) < self.P.p:
            t["status"] = LC_NOT_ENOUGH_IMAGES
            return t["status"], 0
        new_id = self.queue.pop(0)
        t["add_matches"] = self._add_image(new_id, self.prev_descs[new_id])
        t["added"], t["purged"], t["nwords"] = list(self.index.added), list(self.index.purged), len(self.index.words)
        if image_id < self.last_query_id + self.P.nframes_after_lc:
            t["status"] = LC_NOT_ENOUGH_IMAGES
            return t["status"], 0
        matches = self.filter_matches(self.index.search(descs))
        t["matches"] = matches
        score = self.index.search_images(len(descs), matches)
        t["scores"] = list(score)
        order = sorted(range(len(score)), key=lambda i: (-score[i], i))
        margin = _min_gap([score[i] for i in order])
        # filterCandidates, lcdetector.cc:183-204
        mx, mn = score[order[0]], score[order[-1]]
        filt = []
        for i in order:
            new = (score[i] - mn) / (mx - mn) if mx != mn else float("nan")   # 0 / 0 in the reference
            if new == new:
                margin = min(margin, abs(new - self.P.min_score))
            if new > self.P.min_score:
                filt.append((i, new))
            else:
                break
        islands = build_islands(filt, self.P.island_size)
        t["islands"] = [s.tuple() for s in islands]
        t["margin"] = min(margin, _min_gap([s.score for s in islands]))
        if not islands:
            t["status"] = LC_NOT_ENOUGH_ISLANDS
            return t["status"], 0
        prior = [s for s in islands if self.last_island.overlaps(s)]
        island = prior[0] if prior else islands[0]
        self.last_island = island
        self.last_query_id = image_id
        t["status"], t["train_id"] = LC_DETECTED, island.img_id
        return LC_DETECTED, island.img_id


def run_stream(det, stream):
    """feeds the keyframes of a synth_lcd stream that offer descriptors (the loop closer skips the others without advancing the
    image id); returns [(keyframe, image id, status, train image id)] and the image-id-to-keyframe list"""
    out, kf_of = [], []
    for kf, descs in enumerate(stream):
        if len(descs) == 0:
            continue
        img = len(kf_of)
        kf_of.append(kf)
        st, tr = det.process(img, descs)
        out.append((kf, img, st, tr))
    return out, kf_of
