"""The 300 extra FAST + BRIEF keypoints of the loop closer (src/loop_closer.cpp:95-134) in the host mirror: extraKeypoints against
tests/fast_ref.py + the oracle's BRIEF, newKeyframe with an image against tests/lcd_ref.py fed the concatenation, the batched
step against single steps with its call counters, and the repeat of the detect call when an image overflows its room."""
import numpy as np
import pytest

import fast_ref as F
import lcd_ref as R

pytestmark = pytest.mark.gpu

LC_PARAMS = dict(p=2, island_size=4, nframes_after_lc=0, purge_descriptors=False)
NEW = 40            # synth_loop: the keyframe that revisits keyframe 2
W, H = 240, 200     # the small raw images: most keypoints of the 752 x 480 scene lie outside, their discs are clipped away


@pytest.fixture(scope="module")
def mods():
    from ov2slam_amd import frontend, host_map, lcd, mapper, synth_fast, synth_loop
    from oracle import oracle_py
    return dict(fe=frontend, hm=host_map, L=lcd, S=synth_fast, SL=synth_loop, O=oracle_py, pat=mapper.random_brief_pattern(3))


def revisit_map(M):
    """synth_loop's scene plus keyframe 1, whose two map points have no descriptor (the closer skips it)"""
    s = M["SL"].make_scene()
    s["kfids"] = [1] + list(s["kfids"])
    s["poses"][1] = np.array([0.05, 0, 0, 0, 0, 0, 1.0])
    s["kps"][1] = dict(lmid=np.array([90001, 90002], np.int32), uv=np.array([[50, 50], [80, 90]], np.float32), kp3d=np.zeros(2, np.uint8))
    return s, M["hm"].LoopMap(s)


def raw_pyramid(M, ctx, imgs):
    fe = M["fe"]
    if len(imgs) == 1:
        return fe.preprocess_image(ctx, imgs[0], use_clahe=False, nklt_pyr_lvl=0)
    h, w = imgs[0].shape
    im = fe.Images(ctx, len(imgs), w, h)
    for b, a in enumerate(imgs):
        im.upload(b, a)
    return fe.preprocess_images(ctx, im, use_clahe=False, nklt_pyr_lvl=0)


def described(s, m, k):
    """(lmid, px) of the keypoints of keyframe k whose map point exists and has a descriptor, in the mirror's order"""
    uv = dict(zip(s["kps"][k]["lmid"].tolist(), s["kps"][k]["uv"]))
    return [(l, uv[l]) for l in m.keypoint_order(k) if l in s["desc"] and l not in s["forget_lm"]]


def expected_extra(M, img, mask_px):
    """checker keypoints -> (xy, resp, desc) of the ones BRIEF describes, row-major; and the count after retainBest"""
    xy, resp = F.detect(img, 20, 2, mask_px, 300)
    if len(xy) == 0:
        return xy, resp, np.zeros((0, 32), np.uint8), 0
    desc, valid = M["O"].describe_brief(img, xy, M["pat"])
    v = valid.astype(bool)
    return xy[v], resp[v], desc[v], len(xy)


def image_for(M, k, b=0):
    return M["S"].noise_blocks_image(W, H, seed=1000 * b + k, amplitude=16)


def closer(M, ctx, m):
    lc = M["L"].LoopCloser(ctx, m, **LC_PARAMS)
    lc.set_brief_pattern(M["pat"])
    return lc


def plant(img, x, y):
    img[y - 4:y + 5, x - 4:x + 5] = 200
    img[y, x] = 40


def test_extra_keypoints(mods, ctx):
    M = mods
    s, m = revisit_map(M)
    lc = closer(M, ctx, m)
    try:
        uv = dict(zip(s["kps"][NEW]["lmid"].tolist(), s["kps"][NEW]["uv"]))
        inside = lambda l: 40 <= uv[l][0] < 752 - 40 and 40 <= uv[l][1] < 480 - 40
        no_desc = next(l for l in s["effects"]["no_desc"] if l in uv and inside(l))   # its map point has no descriptor
        absent = next(l for l in s["effects"]["absent"] if l in uv and inside(l))     # its map point was removed
        masked = next(l for l in s["effects"]["true"] if inside(l))                   # an ordinary described keypoint
        img = M["S"].noise_blocks_image(752, 480, seed=4, amplitude=16)
        dots = {l: (F.cv_round(uv[l][0]), F.cv_round(uv[l][1])) for l in (no_desc, absent, masked)}
        for x, y in dots.values():
            plant(img, x, y)
        want = described(s, m, NEW)
        assert no_desc not in dict(want) and absent not in dict(want) and masked in dict(want) and len(want) > 60
        mask_px = np.array([p for _, p in want], np.float32)
        pyr = raw_pyramid(M, ctx, [img])
        try:
            (job,), stats = M["L"].extra_keypoints([lc], [NEW], pyr, [0])
        finally:
            pyr.release()
        assert stats == dict(detect_calls=1, describe_calls=1)
        assert job["skipped"] == 0 and job["nbkps"] == len(m.keypoint_order(NEW))
        assert np.array_equal(job["mask_xy"], mask_px)          # exactly the described keypoints, in getKeypoints() order
        exy, eresp, edesc, n_det = expected_extra(M, img, mask_px)
        assert job["n_detected"] == n_det >= 300 and len(exy) < n_det   # some lie within 28 px of the border and are dropped
        assert np.array_equal(job["add_xy"], exy) and np.array_equal(job["add_resp"], eresp)
        assert np.array_equal(job["add_desc"], edesc)
        got = {tuple(int(v) for v in p) for p in job["add_xy"]}
        assert dots[no_desc] in got and dots[absent] in got and dots[masked] not in got
        # a keyframe without any described keypoint is skipped in front of the detection
        pyr = raw_pyramid(M, ctx, [img])
        try:
            (job,), stats = M["L"].extra_keypoints([lc], [1], pyr, [0])
        finally:
            pyr.release()
        assert job["skipped"] == 1 and job["nbkps"] == 2 and stats == dict(detect_calls=0, describe_calls=0)
    finally:
        lc.close()
        m.close()


def test_new_keyframe_with_image_feeds_both_sets(mods, ctx):
    M = mods
    s, m = revisit_map(M)
    s3, m3 = revisit_map(M)
    lc, lc3 = closer(M, ctx, m), closer(M, ctx, m3)
    det, det3 = R.LCDetector(R.Params(**LC_PARAMS)), R.LCDetector(R.Params(**LC_PARAMS))
    try:
        img_id = 0
        for k in [k for k in s["kfids"] if k <= NEW]:
            img = image_for(M, k)
            want = described(s, m, k)
            pyr = raw_pyramid(M, ctx, [img])
            try:
                r = lc.new_keyframe_img(k, 77 + k, pyr)
            finally:
                pyr.release()
            r3 = lc3.new_keyframe(k, 77 + k)
            assert r["nbkps"] == len(m.keypoint_order(k))
            if not want:
                assert k == 1 and r["skipped"] == 1 and r["image_id"] == -1 and r["extra"] == dict(detect_calls=0, describe_calls=0)
                assert r3["skipped"] == 1
                continue
            rows = np.stack([s["desc"][l] for l, _ in want])
            exy, _, edesc, _ = expected_extra(M, img, np.array([p for _, p in want], np.float32))
            assert len(exy) > 50
            status, train = det.process(img_id, np.concatenate([rows, edesc]))     # the map points' rows, then the extra ones
            status3, train3 = det3.process(img_id, rows)
            assert r["extra"] == dict(detect_calls=1, describe_calls=1)
            assert (r["skipped"], r["image_id"], r["status"], r["n_extra"], r["n_descs"]) == (0, img_id, status, len(exy), len(rows) + len(exy)), k
            assert (r3["skipped"], r3["image_id"], r3["status"]) == (0, img_id, status3), k
            if status == R.LC_DETECTED:
                assert r["train_id"] == train, k
            if status3 == R.LC_DETECTED:
                assert r3["train_id"] == train3, k
            assert lc.detector_counts()["words"] == len(det.index.words), k      # the index grew by both sets
            assert lc3.detector_counts()["words"] == len(det3.index.words), k    # the three-argument form: map points only
            img_id += 1
        assert img_id >= 4 and len(det.index.words) > len(det3.index.words)
    finally:
        lc.close()
        lc3.close()
        m.close()
        m3.close()


def test_batched_step_equals_single_steps(mods, ctx):
    M = mods
    maps = [revisit_map(M) for _ in range(6)]
    together = [closer(M, ctx, m) for _, m in maps[:3]]
    alone = [closer(M, ctx, m) for _, m in maps[3:]]
    s = maps[0][0]
    try:
        ks = [k for k in s["kfids"] if k <= NEW]
        # closer b sees the keyframes shifted by b places, so that a step mixes skipped, ordinary and detecting closers
        most = 0
        for step in range(len(ks) + 2):
            act = [b for b in range(3) if 0 <= step - b < len(ks)]
            kf = [ks[step - b] for b in act]
            imgs = [image_for(M, ks[step - b], b) for b in act]
            pyr = raw_pyramid(M, ctx, imgs)
            try:
                c0 = M["L"].search_calls(ctx)
                res = M["L"].new_keyframes([together[b] for b in act], kf, [7 + k for k in kf], pyr, list(range(len(act))))
                calls = M["L"].search_calls(ctx) - c0
            finally:
                pyr.release()
            n_live = sum(1 for r in res if not r["skipped"])
            for r in res:
                assert r["extra"] == (dict(detect_calls=1, describe_calls=1) if n_live else dict(detect_calls=0, describe_calls=0)), step
            single_calls = 0
            for i, b in enumerate(act):
                pyr = raw_pyramid(M, ctx, [imgs[i]])
                try:
                    c0 = M["L"].search_calls(ctx)
                    one = alone[b].new_keyframe_img(kf[i], 7 + kf[i], pyr)
                    single_calls += M["L"].search_calls(ctx) - c0
                finally:
                    pyr.release()
                a, o = dict(res[i]), dict(one)
                a.pop("extra"), o.pop("extra")
                assert a == o, (step, b)
                assert together[b].detector_counts() == alone[b].detector_counts(), (step, b)
            # LCDetector::processBatch: one search for the delayed images' addImage and one for the queries, whatever B is
            assert calls <= 2 and calls <= single_calls, step
            most = max(most, single_calls)
        assert most > 2   # a step where the single closers together needed more searches than the batch's two
    finally:
        for lc in together + alone:
            lc.close()
        for _, m in maps:
            m.close()


def test_overflow_repeats_the_detect_call_once(mods, ctx):
    M = mods
    s, m = revisit_map(M)
    lc = closer(M, ctx, m)
    try:
        img = M["S"].motif_image(21, 20)   # 420 keypoints of one response: retainBest(300) keeps them all
        pyr = raw_pyramid(M, ctx, [img])
        try:
            (full,), stats = M["L"].extra_keypoints([lc], [NEW], pyr, [0])
            assert stats == dict(detect_calls=1, describe_calls=1) and full["n_detected"] > 300
            lc.set_extra_cap(64)
            (small,), stats = M["L"].extra_keypoints([lc], [NEW], pyr, [0])
        finally:
            pyr.release()
        assert stats == dict(detect_calls=2, describe_calls=1)
        assert full.keys() == small.keys()
        for key in full:
            assert np.array_equal(full[key], small[key]), key
        exy, eresp, edesc, n_det = expected_extra(M, img, np.array([p for _, p in described(s, m, NEW)], np.float32))
        assert small["n_detected"] == n_det and np.array_equal(small["add_xy"], exy) and np.array_equal(small["add_desc"], edesc)
    finally:
        lc.close()
        m.close()
