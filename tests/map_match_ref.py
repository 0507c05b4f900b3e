"""numpy checker of the match gather (ov2_map_match_gather_batch_dev, csrc/map.hip): a model of the map mirror's tables with
the match columns -- one row per observation with its raw pixel and, maybe, a descriptor -- that takes the same edits as the
mirror and lists, for a new keyframe, what Mapper::matchToMap reads (src/mapper.cpp:576-774) as the flat arrays of
mapper.MatchBatchInput.  Written from the header's description of the entry point, not from the kernels: plain loops over rows.

Edits (tuples, applied in order by Model.apply):
  ("remove_obs", kfid, lmid)            MapManager::removeMapPointObs: the live row (kfid, lmid) dies, with its descriptor
  ("remove_keyframe", kfid)             MapManager::removeKeyframe: a keyframe that is not alive has no live rows
  ("remove_landmarks", [lmid, ...])     MapManager::removeMapPoint
  ("append", kfid, lmid, px, desc)      a row appended to a keyframe already in the map; desc = None: no descriptor
  ("set_desc", kfid, lmid, desc)        MapPoint::addDesc for an observing keyframe
  ("merge", [(prev, new), ...])         MapManager::mergeMapPoints per pair, in list order, with the conflict rule: where the
                                        keyframe holds prev and new, new's row takes prev's descriptor iff it has none"""
import numpy as np

from ov2slam_amd import device_map as DM, mapper, synth_match as SM

LM_ALIVE, LM_3D = DM.LM_ALIVE, DM.LM_3D


class Model:
    def __init__(self, s):
        """from a synth_revisit.make_local_map_scene dict, as DeviceMap.from_scene fills the mirror"""
        rows = DM.scene_rows(s)
        self.kf, self.lm, self.px, self.desc, self.has, self.alive = [], [], [], [], [], []
        self.pose, self.kf_alive = {}, set()
        for k in s["kfids"]:
            self.pose[int(k)] = np.asarray(s["poses"][k], np.float64).copy()
            self.kf_alive.add(int(k))
            r = rows[k]
            for i in range(len(r["lmid"])):
                self._row(int(k), int(r["lmid"][i]), r["px"][i], r["desc"][i] if r["has_desc"][i] else None)
        lmid, xyz, state = DM.scene_landmarks(s)
        self.state = {int(l): int(st) for l, st in zip(lmid, state)}
        self.xyz = {int(l): np.asarray(x, np.float64) for l, x in zip(lmid, xyz)}

    def _row(self, kf, lm, px, desc):
        self.kf.append(kf); self.lm.append(lm); self.px.append(np.float32(px).copy()); self.alive.append(True)
        self.has.append(desc is not None)
        self.desc.append(np.zeros(32, np.uint8) if desc is None else np.asarray(desc, np.uint8).copy())

    def _live(self, i):
        return self.alive[i] and self.kf[i] in self.kf_alive and bool(self.state.get(self.lm[i], 0) & LM_ALIVE)

    def live_rows(self, lm):
        """the live rows of a landmark, in table order"""
        return [i for i in range(len(self.kf)) if self.lm[i] == lm and self._live(i)]

    def apply(self, edits):
        for e in edits:
            op = e[0]
            if op == "remove_obs":
                for i in range(len(self.kf)):
                    if self.alive[i] and self.kf[i] == e[1] and self.lm[i] == e[2]:
                        self.alive[i] = False
            elif op == "remove_keyframe":
                self.kf_alive.discard(int(e[1]))
            elif op == "remove_landmarks":
                for l in e[1]:
                    self.state[int(l)] = 0
            elif op == "append":
                self._row(int(e[1]), int(e[2]), e[3], e[4])
            elif op == "set_desc":
                for i in range(len(self.kf)):
                    if self.alive[i] and self.kf[i] == e[1] and self.lm[i] == e[2]:
                        self.desc[i], self.has[i] = np.asarray(e[3], np.uint8).copy(), True
            elif op == "merge":
                for p, n in e[1]:
                    self._merge(int(p), int(n))
            else:
                raise ValueError(op)
        return self

    def _merge(self, p, n):
        sp, sn = self.state.get(p, 0), self.state.get(n, 0)
        if p == n or not (sp & LM_ALIVE) or not (sn & LM_ALIVE) or not (sn & LM_3D):
            return
        new_row = {self.kf[i]: i for i in self.live_rows(n)}
        for i in self.live_rows(p):
            j = new_row.get(self.kf[i])
            if j is None:
                self.lm[i] = n                      # Frame::updateKeypointId: the row moves, pixel and descriptor with it
            elif self.has[i] and not self.has[j]:   # conflict: addDesc(kfid, prev's descriptor) finds none under that keyframe
                self.desc[j], self.has[j] = self.desc[i].copy(), True
        self.state[p] = 0

    def _observers(self, lm):
        rows = sorted(self.live_rows(lm), key=lambda i: self.kf[i])    # MapPoint::set_kfids_: ascending
        return rows, [self.desc[i] for i in rows if self.has[i]]

    def frame(self, newkf, kp_lmid, cand_lmid, nb3dkps, max_kf):
        """the dict mapper.MatchBatchInput takes for one frame; max_kf: rows of the pose table (the mirror's keyframe capacity)"""
        kps, cands = [], []
        empty = dict(descs=np.zeros((0, 32), np.uint8), kfids=[], kf_px=np.zeros((0, 2), np.float32))
        for l in kp_lmid:
            alive = bool(self.state.get(int(l), 0) & LM_ALIVE)
            rows, descs = self._observers(int(l)) if alive else ([], [])
            own = [i for i in rows if self.kf[i] == newkf]
            k = dict(empty, px=self.px[own[0]] if own else np.zeros(2, np.float32))
            if descs:
                k.update(descs=np.array(descs, np.uint8), kfids=[self.kf[i] for i in rows], kf_px=np.array([self.px[i] for i in rows], np.float32))
            kps.append(k)
        for l in cand_lmid:
            st = self.state.get(int(l), 0)
            alive = bool(st & LM_ALIVE)
            rows, descs = self._observers(int(l)) if alive else ([], [])
            c = dict(wpt=self.xyz[int(l)] if alive else np.zeros(3), descs=np.zeros((0, 32), np.uint8), kfids=[])
            if alive and (st & LM_3D) and descs and not any(self.kf[i] == newkf for i in rows):
                c.update(descs=np.array(descs, np.uint8), kfids=[self.kf[i] for i in rows])
            cands.append(c)
        kf_Twc = np.zeros((max_kf, 7))
        for k, T in self.pose.items():
            kf_Twc[k] = T
        return dict(Twc=self.pose[newkf], kps=kps, cands=cands, kf_Twc=kf_Twc, nb3dkps=int(nb3dkps))


def scene_lists(s):
    """(newkf, keypoint lmids of the new keyframe in the scene's order, the unfiltered local ids) of a synth_match.local_map_scenes map"""
    newkf = int(s["pairs"]["revisit"][0])
    return newkf, [int(l) for l in s["kps"][newkf]["lmid"]], [int(l) for l in s["local"]]


def batch_input(frames):
    """the flat arrays of the frames with the scenes' camera"""
    return mapper.MatchBatchInput(frames, SM.K4, SM.W, SM.H, SM.CELL, [f["nb3dkps"] for f in frames])


def single_input(f):
    return mapper.MatchInput(f["Twc"], SM.K4, SM.W, SM.H, SM.CELL, f["nb3dkps"], f["kps"], f["cands"], f["kf_Twc"])
