"""Checker of the loop closer's map matcher: LoopCloser::matchToMap (src/loop_closer.cpp:586-763) restated in numpy / python on
the pair dicts of ov2slam_amd/synth_revisit.py (float32 where the reference holds floats).  The keypoint order (it fills
Frame::vgridkps_ and decides best / second best ties) and the candidate order (the reference walks an unordered_set; it decides
ties between candidates) are INPUTS: the order of the two lists.

Besides the matches it returns a trace: how often each gate fired, and the margin of every float gate decision (pixel
distance, z, view angle, image border, and the cell boundary next to the projection), so that a test can assert that no
decision hangs on the last bits of a projection."""
import numpy as np

f32, f64 = np.float32, np.float64


def pose_R(T):
    """rotation of a pose [t, qx qy qz qw]: the quaternion normalised, then Eigen's toRotationMatrix"""
    q = np.asarray(T[3:7], f64)
    x, y, z, w = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def thresholds(K, img_w, img_h, fmaxprojerr, fdistratio):
    """(dmaxpxdist, mindist, view_th) AS WRITTEN at :595-607 and :656: vfov / hfov are products, atan(hfov) in both branches"""
    hfov = f32(0.5 * f64(img_w) * f64(K[0]))
    view_th = np.cos(np.arctan(hfov, dtype=f32), dtype=f32)
    return f32(fmaxprojerr), f32(f64(f32(32) * f32(fdistratio)) * 8.0), view_th


def project_dist(K, campt, cam=None):
    """Frame::projCamToImageDist: pinhole, or radial-tangential (cam = (k1, k2, p1, p2[, k3])) on a Point2f as cv::projectPoints"""
    x, y = campt[0] * (1.0 / campt[2]), campt[1] * (1.0 / campt[2])
    if cam is None:
        return f32(K[0] * x + K[2]), f32(K[1] * y + K[3])
    k1, k2, p1, p2 = cam[:4]
    k3 = cam[4] if len(cam) > 4 else 0.0
    xf, yf = f64(f32(x)), f64(f32(y))
    r2 = xf * xf + yf * yf
    r4, r6 = r2 * r2, r2 * r2 * r2
    a1, a2, a3 = 2 * xf * yf, r2 + 2 * xf * xf, r2 + 2 * yf * yf
    cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
    xd, yd = xf * cdist + p1 * a1 + p2 * a2, yf * cdist + p1 * a3 + p2 * a1
    return f32(xd * K[0] + K[2]), f32(yd * K[1] + K[3])


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def loop_match_to_map(pair, K, img_w, img_h, cell, fmaxprojerr, fdistratio, cam=None):
    """returns (match_cand (n_kp,) int32: index into pair["cands"] or -1, match_dist (n_kp,) f32, trace)"""
    kps, cands = pair["kps"], pair["cands"]
    n_kp = len(kps)
    mc, md = np.full(n_kp, -1, np.int32), np.zeros(n_kp, f32)
    tr = dict(n=dict(cand_nodesc=0, z_under=0, behind=0, view=0, outside=0, row0=0, col0=0, last_cell=0, cell_gt64=0, cell_gt128=0,
                     kp_masked=0, kp_nodesc=0, px_over=0, px_under=0, coobs=0, min_not_first=0, ratio_reject=0, best_late_chunk=0,
                     later_wins=0, offered=0),
              m_px=[], m_z=[], m_view=[], m_border=[], m_cell=[])
    if n_kp == 0 or len(cands) == 0:     # :591-593
        return mc, md, tr
    dmax, mindist, view_th = thresholds(K, img_w, img_h, fmaxprojerr, fdistratio)
    nbw, nbh = int(np.ceil(f32(img_w) / f32(cell))), int(np.ceil(f32(img_h) / f32(cell)))
    cells = [[] for _ in range(nbw * nbh)]
    for i, k in enumerate(kps):
        cells[int(np.floor(f32(k["px"][1]) / f32(cell))) * nbw + int(np.floor(f32(k["px"][0]) / f32(cell)))].append(i)
    R, t = pose_R(pair["Twc"]), np.asarray(pair["Twc"][:3], f64)
    per_kp = {}
    N = tr["n"]
    for c, q in enumerate(cands):
        if len(q["descs"]) == 0:
            N["cand_nodesc"] += 1
            continue
        campt = R.T @ (np.asarray(q["wpt"], f64) - t)
        tr["m_z"].append(abs(campt[2] - 0.1))
        if campt[2] < 0.1:
            N["behind" if campt[2] < 0 else "z_under"] += 1
            continue
        va = f32(campt[2] / np.sqrt((campt * campt).sum()))
        tr["m_view"].append(abs(f64(abs(va)) - f64(view_th)))
        if abs(va) < view_th:
            N["view"] += 1
            continue
        px, py = project_dist(K, campt, cam)
        tr["m_border"].append(min(abs(f64(px)), abs(f64(py)), abs(f64(px) - img_w), abs(f64(py) - img_h)))
        if not (px >= 0 and py >= 0 and px < img_w and py < img_h):
            N["outside"] += 1
            continue
        N["offered"] += 1
        rkp, ckp = int(np.floor(py / f32(cell))), int(np.floor(px / f32(cell)))
        tr["m_cell"].append(min(f64(px) - ckp * cell, (ckp + 1) * cell - f64(px), f64(py) - rkp * cell, (rkp + 1) * cell - f64(py)))
        N["row0"] += rkp == 0
        N["col0"] += ckp == 0
        N["last_cell"] += rkp * nbw + ckp == nbw * nbh - 1
        best, sec, bd, sd, pos, bestpos = -1, -1, mindist, mindist, 0, -1
        for r in (rkp - 1, rkp):
            for cc in (ckp - 1, ckp):
                idx = r * nbw + cc
                if r < 0 or cc < 0 or idx >= nbw * nbh:
                    continue
                N["cell_gt64"] += len(cells[idx]) > 64
                N["cell_gt128"] += len(cells[idx]) > 128
                for pos, k in enumerate(cells[idx]):
                    kp = kps[k]
                    if kp["matched"]:                      # :672-675, before the pixel gate
                        N["kp_masked"] += 1
                        continue
                    dx, dy = f32(px - kp["px"][0]), f32(py - kp["px"][1])
                    pxdist = f32(np.sqrt(f64(dx) * f64(dx) + f64(dy) * f64(dy)))
                    tr["m_px"].append(abs(f64(pxdist) - f64(dmax)))
                    if pxdist > dmax:
                        N["px_over"] += 1
                        continue
                    N["px_under"] += 1
                    if len(kp["descs"]) == 0:              # :690-695
                        N["kp_nodesc"] += 1
                        continue
                    if set(kp["kfids"]) & set(q["kfids"]):
                        N["coobs"] += 1
                        continue
                    allh = [[hamming(a, b) for b in kp["descs"]] for a in q["descs"]]
                    dist = f32(min(min(row) for row in allh))
                    N["min_not_first"] += dist < allh[0][0]
                    if dist <= bd:
                        sd, sec, bd, best, bestpos = bd, best, dist, k, pos
                    elif dist <= sd:
                        sd, sec = dist, k
        if best != -1 and sec != -1 and 0.9 * f64(sd) < f64(bd):
            N["ratio_reject"] += 1
            best = -1
        if best < 0:
            continue
        N["best_late_chunk"] += bestpos >= 64
        per_kp.setdefault(best, []).append((c, bd))
    for k, lst in per_kp.items():     # :743-760
        b, bl = f32(1024), -1
        for c, dd in lst:
            if dd <= b:
                N["later_wins"] += bl >= 0 and dd == b
                b, bl = dd, c
        mc[k], md[k] = bl, b
    return mc, md, tr


def assemble_loop_local_map(s, order, newkf, lckf, vkplmids):
    """LoopCloser::trackLoopLocalMap in front of its matcher (src/loop_closer.cpp:502-568) and the candidate filter of
    :612-631, on a scene dict of synth_revisit.make_local_map_scene.  order[k]: the lmids of keyframe k in the order the map
    under test iterates its keypoints (an input: the reference's containers leave it open).  The local set is kept in ORDER OF
    FIRST ENCOUNTER.  returns dict(vkplmids, n_identity, matched, local, cands)"""
    in_map = set(s["kfids"])
    kp3d = {k: dict(zip(v["lmid"].tolist(), v["kp3d"].tolist())) for k, v in s["kps"].items()}
    exists, is3d = set(), {}
    for k in s["kfids"]:                                   # a map point is created by the first keyframe that names it
        for l, f in zip(s["kps"][k]["lmid"].tolist(), s["kps"][k]["kp3d"].tolist()):
            if l not in is3d:
                is3d[l] = bool(f)
            exists.add(l)
    exists -= set(s["forget_lm"])
    cov = {b: sc for a, b, sc in s["cov"] if a == lckf}
    cov[lckf] = 100
    new_obs = set(s["kps"][newkf]["lmid"].tolist())
    pairs = [tuple(p) for p in vkplmids]
    checked, local, n_identity = set(), [], 0
    for kfid in sorted(cov):
        if kfid < lckf - 15:
            continue
        if kfid > lckf + 15:
            break
        if kfid not in in_map:
            continue
        for l in order[kfid]:
            if not kp3d[kfid][l] or l in checked:
                continue
            checked.add(l)
            if l in new_obs:
                if (l, l) not in pairs:
                    pairs.append((l, l))
                    n_identity += 1
            else:
                local.append(l)
    seconds = set(p[1] for p in pairs)
    local = [l for l in local if l not in seconds]
    cands = [l for l in local if l not in new_obs and l in exists and is3d[l] and l in s["desc"]]
    return dict(vkplmids=pairs, n_identity=n_identity, matched=[p[0] for p in pairs], local=local, cands=cands)


def track_pair(s, order, newkf, r):
    """the matcher's pair dict (keypoints of newkf in the order the map iterates them, candidates in r["cands"] order) for a
    scene of synth_revisit.make_local_map_scene after assemble_loop_local_map returned r, and the lmid of every entry"""
    gone = set(s["forget_lm"])
    obs = {}
    for k in s["kfids"]:
        for l in s["kps"][k]["lmid"].tolist():
            obs.setdefault(l, set()).add(k)

    def descs_of(l):
        if l in gone or l not in s["desc"]:
            return np.zeros((0, 32), np.uint8)
        return np.stack([s["desc"][l]] + [d for _, d in s.get("descs", {}).get(l, [])])
    uv = dict(zip(s["kps"][newkf]["lmid"].tolist(), s["kps"][newkf]["uv"]))
    matched = set(r["matched"])
    kps = [dict(px=uv[l], matched=l in matched, descs=descs_of(l), kfids=sorted(obs[l]) if len(descs_of(l)) else [], lmid=l)
           for l in order[newkf]]
    cands = [dict(wpt=s["wpt"][l], descs=descs_of(l), kfids=sorted(obs[l]), lmid=l) for l in r["cands"]]
    return dict(Twc=s["Twc"], kps=kps, cands=cands)


def track_loop_local_map(s, order, newkf, lckf, vkplmids, K, img_w, img_h, cell, maxdist, ratio, Twc=None):
    """LoopCloser::trackLoopLocalMap (src/loop_closer.cpp:502-583): assemble, match, append the new pairs in ascending keypoint
    lmid (the reference's std::map).  returns dict(vkplmids, n_identity, n_offered, n_matched, trace)"""
    r = assemble_loop_local_map(s, order, newkf, lckf, vkplmids)
    pair = track_pair(s, order, newkf, r)
    if Twc is not None:
        pair["Twc"] = Twc
    mc, _, tr = loop_match_to_map(pair, K, img_w, img_h, cell, maxdist, ratio)
    new = sorted((pair["kps"][k]["lmid"], pair["cands"][c]["lmid"]) for k, c in enumerate(mc.tolist()) if c >= 0)
    return dict(vkplmids=r["vkplmids"] + new, n_identity=r["n_identity"], n_offered=len(r["cands"]), n_matched=len(new), trace=tr)


def compute_pnp(pnp_solve, s, newkf, vkplmids, Twc0, K, voutlier_idx=()):
    """LoopCloser::computePnP (src/loop_closer.cpp:834-897) on a scene of synth_revisit.make_local_map_scene; pnp_solve: the
    CPU oracle's ceresPnP passed in as a function (as p3p_ref.compute_pose takes it).  Pairs whose map point is gone or whose
    keypoint the frame does not hold stay out; the solver's outliers are mapped back through vgoodkpidx and APPENDED.
    returns (success, Twc, voutlier_idx, vgoodkpidx)"""
    gone = set(s["forget_lm"])
    uv = dict(zip(s["kps"][newkf]["lmid"].tolist(), s["kps"][newkf]["uv"]))
    good = [i for i, (kpid, lmid) in enumerate(vkplmids) if lmid in s["wpt"] and lmid not in gone and kpid in uv]
    out = list(voutlier_idx)
    if len(good) < 3:
        return False, np.array(Twc0, f64), out, good
    unpx = np.array([uv[vkplmids[i][0]] for i in good], f32).astype(f64)           # no distortion: unpx_ = px_
    wpts = np.array([s["wpt"][vkplmids[i][1]] for i in good], f64)
    Kf = [float(f32(v)) for v in K]                                                # ceresPnP takes fx, fy, cx, cy as floats
    ok, T, mask, _ = pnp_solve(unpx, wpts, Kf, Twc0, np.zeros(len(good), np.int32), 10, float(f32(5.9915)), True, False)
    return bool(ok), T, out + [good[i] for i in np.flatnonzero(mask)], good


LV_P3P_FAILED, LV_NO_NEW_MATCHES, LV_PNP_FAILED, LV_FEW_GOOD, LV_ACCEPTED = range(5)      # ov2::LoopVerifyBranch
# Tolerance of the GPU tests on both poses of a verify result.  tests/test_loop_verify_ref_cpu.py::test_tameness re-runs the checker with
# the pose after P3P + refinement perturbed by +-1e-8 per component: the integers, lists, branches and masks do not change and the
# largest change of the final Twc over those runs is MEASURED there as 1.0e-8 (the solve ends where it starts within its own
# tolerances, so the perturbation passes through).  10 x that spread covers the P3P parity band of 1e-8 (tests/test_p3p_gpu.py) plus
# ceresPnP's own 1e-9.  The CPU test fails if the measured spread no longer supports this constant (in either direction).
POSE_SPREAD_MEASURED, POSE_TOL = 1.0e-8, 1.0e-7
SEED = 11              # chosen on the checker: every RANSAC gap of the seven named pairs exceeds test_p3p_gpu.GAP = 1e-6


def se3_log_norm(Ta, Tb):
    """|log(Ta^-1 * Tb)| of two poses [t, q] (Sophus::SE3::log, tangent [upsilon, omega])"""
    Ra, Rb = pose_R(Ta), pose_R(Tb)
    R, t = Ra.T @ Rb, Ra.T @ (np.asarray(Tb[:3], f64) - np.asarray(Ta[:3], f64))
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-10:
        return float(np.linalg.norm(t))
    w = th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Vinv = np.eye(3) - 0.5 * O + (1 - th * np.cos(th / 2) / (2 * np.sin(th / 2))) / th ** 2 * O @ O
    return float(np.linalg.norm(np.concatenate([Vinv @ t, w])))


def p3p_stage(pnp_solve, s, newkf, vkplmids, K, nransac_iter, errth, seed):
    """LoopCloser::p3pRansac (src/loop_closer.cpp:765-831) with the refinement that stands for OpenGV's do_optimize: the vbadidx
    erasure, < 4 -> false, RANSAC with 10 * nransac_iter draws, then a motion-only solve on the inliers with bz > 0 (pixels
    (fx bx / bz, fy by / bz), K = (fx, fy, 0, 0), 10 iterations, robust, no L2 re-solve; its flags ignored; kept only on success).
    returns dict(success, pairs: the list after the erasure, outliers: indices into it, Twc or None, Twc_ransac, status, info, gaps)"""
    import p3p_ref as PR
    from epipolar_ref import bearing
    res = dict(success=False, pairs=list(vkplmids), outliers=[], Twc=None, Twc_ransac=None, status=-1, info=[0, 0, -1, 0], gaps=None)
    if len(vkplmids) < 4:
        return res
    gone = set(s["forget_lm"])
    uv = dict(zip(s["kps"][newkf]["lmid"].tolist(), s["kps"][newkf]["uv"]))
    pairs = [p for p in vkplmids if p[1] in s["wpt"] and p[1] not in gone]
    res["pairs"] = pairs
    if len(pairs) < 4:
        return res
    bv = np.array([bearing(uv[q], K) for q, _ in pairs])
    X = np.array([s["wpt"][l] for _, l in pairs])
    fx, fy = float(f32(K[0])), float(f32(K[1]))
    r = PR.p3p_ransac(bv, X, [fx, fy, 0., 0.], 10 * nransac_iter, errth, False, seed)
    res.update(status=int(r["status"]), info=[int(v) for v in r["info"]], gaps=r["gaps"])
    if r["status"] != 1:
        return res
    T = np.array(r["Twc"], f64)
    res["Twc_ransac"] = T.copy()
    use = (~r["outlier"]) & (bv[:, 2] > 0)
    unpx = np.stack([fx * bv[use, 0] / bv[use, 2], fy * bv[use, 1] / bv[use, 2]], 1)
    ok, Tr, _, _ = pnp_solve(unpx, X[use], [fx, fy, 0., 0.], T, None, 10, float(f32(5.9915)), True, False)
    res.update(success=True, outliers=np.flatnonzero(r["outlier"]).tolist(), Twc=np.array(Tr, f64) if ok else T)
    return res


def verify_loop_candidate(pnp_solve, s, order, newkf, lckf, vkplmids, seed, K, img_w, img_h, cell, maxdist, ratio,
                          nransac_iter=100, errth=3.0, perturb=None):
    """LoopCloser::processLoopCandidate :238-300 on a make_local_map_scene map.  perturb (7,): added to the pose after P3P +
    refinement (the tameness runs).  returns dict(branch, p3p_status, p3p_info, after_p3p, after_track, final, n_identity,
    n_offered, n_matched, Twc_p3p, Twc, lc_pose_err, pnp_outliers, gaps)"""
    from loop_ref import remove_outliers
    out = dict(branch=LV_P3P_FAILED, p3p_status=-1, p3p_info=[0, 0, -1, 0], after_p3p=[], after_track=[], final=[], n_identity=0,
               n_offered=0, n_matched=0, Twc_p3p=None, Twc=None, lc_pose_err=0.0, pnp_outliers=[], gaps=None)
    p = p3p_stage(pnp_solve, s, newkf, [tuple(x) for x in vkplmids], K, nransac_iter, errth, seed)
    out.update(p3p_status=p["status"], p3p_info=p["info"], gaps=p["gaps"])
    nbinliers = len(p["pairs"]) - len(p["outliers"])
    if not p["success"] or nbinliers < 5:                                            # :251
        return out
    pairs = remove_outliers(p["pairs"], p["outliers"])                               # :260-263
    Twc = p["Twc"] if perturb is None else p["Twc"] + np.asarray(perturb)
    out.update(after_p3p=list(pairs), Twc_p3p=np.array(Twc))
    t = track_loop_local_map(s, order, newkf, lckf, pairs, K, img_w, img_h, cell, maxdist, ratio, Twc=Twc)   # :269
    pairs = t["vkplmids"]
    out.update(after_track=list(pairs), n_identity=t["n_identity"], n_offered=t["n_offered"], n_matched=t["n_matched"], trace=t["trace"])
    out["branch"] = LV_NO_NEW_MATCHES
    if not len(pairs) > nbinliers:                                                   # :275, :298-300
        return out
    ok, T, outl, _ = compute_pnp(pnp_solve, s, newkf, pairs, Twc, K, [])             # :277
    out.update(pnp_outliers=list(outl), Twc=np.array(T), branch=LV_PNP_FAILED)
    nbinliers = len(pairs) - len(outl)
    if not ok or nbinliers < 30:                                                     # :288
        return out
    pairs = remove_outliers(pairs, outl)                                             # :294-297
    out["final"] = list(pairs)
    out["branch"] = LV_ACCEPTED if len(pairs) >= 30 else LV_FEW_GOOD                 # :305
    out["lc_pose_err"] = se3_log_norm(s["poses"][newkf], T)                          # :318 |log(Tcw_new * Twc)|
    return out
