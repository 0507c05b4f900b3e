"""Host-side mirror of the reference's static MultiViewGeometry helpers (ceresPnP, compute5ptEssentialMatrix, p3pRansac,
triangulate; reference include/multi_view_geometry.hpp, src/multi_view_geometry.cpp) over the C ABI.  The solves run in HIP
kernels (csrc/pnp.hip, epipolar.hip, p3p.hip, tri.hip); this file only marshals arrays.  No arithmetic happens here."""
import numpy as np

from .frontend import _check


def _vp(a):
    return a.ctypes.data


class MultiViewGeometry:
    """mirror of the reference's static MultiViewGeometry helpers for the pose-refinement path."""

    def __init__(self, ctx):
        self.ctx = ctx

    def ceresPnP(self, vunkps, vwpts, Twc, nmaxiter, chi2th, buse_robust, bapply_l2_after_robust, fx, fy, cx, cy,
                 vscales=None):
        """one frame.  returns (success, Twc (7,) [t, qx qy qz qw], voutliersidx (sorted int array))."""
        ok, T, out, _ = self.ceresPnP_batch([vunkps], [vwpts], np.asarray(Twc, np.float64).reshape(1, 7), nmaxiter,
                                            chi2th, buse_robust, bapply_l2_after_robust,
                                            np.array([[fx, fy, cx, cy]], np.float64),
                                            None if vscales is None else [vscales])
        return bool(ok[0]), T[0], np.flatnonzero(out[0]).astype(np.int32)

    def triangulate_pairs(self, T_ab, bv_a, bv_b, unpx_a, unpx_b, K_a, K_b, max_reproj_err, method=0, Twc_a=None, grp=None,
                          want_parallax=False):
        """per-keypoint bodies of Mapper::triangulateStereo / triangulateTemporal (src/mapper.cpp:191-461) through
        ov2_triangulate_pairs: MultiViewGeometry::triangulate (mid-point, method 0) or the rectified disparity form
        (method 1) + depth / reprojection gates + world projection + parallax. returns dict(pt_a, wpt, parallax, status)."""
        T_ab = np.ascontiguousarray(T_ab, np.float64).reshape(-1, 7)
        bv_a, bv_b = np.ascontiguousarray(bv_a, np.float64).reshape(-1, 3), np.ascontiguousarray(bv_b, np.float64).reshape(-1, 3)
        if len(bv_a) != len(bv_b):
            raise ValueError("bv_a / bv_b sizes differ")
        ua, ub = np.ascontiguousarray(unpx_a, np.float32).reshape(-1, 2), np.ascontiguousarray(unpx_b, np.float32).reshape(-1, 2)
        n = len(bv_a)
        W = None if Twc_a is None else np.ascontiguousarray(Twc_a, np.float64).reshape(-1, 7)
        g = None if grp is None else np.ascontiguousarray(grp, np.int32)
        Ka, Kb = np.ascontiguousarray(K_a, np.float64), np.ascontiguousarray(K_b, np.float64)
        pt, st = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.uint8)
        wpt = None if W is None else np.zeros((max(n, 1), 3))
        par = np.zeros(max(n, 1)) if want_parallax else None
        c = self.ctx
        _check(c.h, c.lib.ov2_triangulate_pairs(c.h, n, int(method), len(T_ab), _vp(T_ab), None if W is None else _vp(W),
                                                None if g is None else _vp(g), _vp(bv_a), _vp(bv_b), _vp(ua), _vp(ub), _vp(Ka),
                                                _vp(Kb), float(max_reproj_err), _vp(pt), None if wpt is None else _vp(wpt),
                                                None if par is None else _vp(par), _vp(st)))
        return dict(pt_a=pt[:n], wpt=None if wpt is None else wpt[:n], parallax=None if par is None else par[:n], status=st[:n])

    def ceresPnP_batch_dev(self, B, d_off, d_unpx, d_wpts, d_scales, d_K, d_Twc, nmaxiter, chi2th, buse_robust,
                           bapply_l2_after_robust, d_outlier, d_removed, d_success, d_iters=None):
        """device-resident, asynchronous form (ov2_pnp_solve_batch_dev): DeviceArrays in, nothing synchronised."""
        p = lambda a: None if a is None else a.ptr
        c = self.ctx
        _check(c.h, c.lib.ov2_pnp_solve_batch_dev(c.h, int(B), p(d_off), p(d_unpx), p(d_wpts), p(d_scales), p(d_K), p(d_Twc),
                                                  int(nmaxiter), float(chi2th), int(bool(buse_robust)),
                                                  int(bool(bapply_l2_after_robust)), p(d_outlier), p(d_removed),
                                                  p(d_success), p(d_iters)))

    def ceresPnP_batch(self, unpx_list, wpts_list, Twc, nmaxiter, chi2th, buse_robust, bapply_l2_after_robust, K,
                       scales_list=None):
        """B independent frames in one launch (one workgroup each).
        returns (success (B,) bool, Twc (B,7), [outlier mask per frame], iters (B,2))."""
        B = len(unpx_list)
        n_pts = np.array([len(u) for u in unpx_list], np.int32)
        cat = lambda xs, k, dt: (np.concatenate([np.asarray(x, dt).reshape(-1, k) for x in xs]) if B and n_pts.sum()
                                 else np.zeros((0, k), dt))
        unpx = np.ascontiguousarray(cat(unpx_list, 2, np.float64))
        wpts = np.ascontiguousarray(cat(wpts_list, 3, np.float64))
        if len(wpts) != len(unpx):
            raise ValueError("vunkps.size() != vwpts.size()")       # the reference asserts (:500)
        sc = None if scales_list is None else np.ascontiguousarray(cat(scales_list, 1, np.int32).ravel())
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(B, 4))
        T = np.ascontiguousarray(np.array(Twc, np.float64).reshape(B, 7))
        n = int(n_pts.sum())
        outl = np.zeros(max(n, 1), np.uint8)
        ok = np.zeros(max(B, 1), np.int32)
        it = np.zeros((max(B, 1), 2), np.int32)
        c = self.ctx
        _check(c.h, c.lib.ov2_pnp_solve_batch(c.h, B, _vp(n_pts) if B else None, _vp(unpx) if n else None,
                                              _vp(wpts) if n else None, None if sc is None or not n else _vp(sc),
                                              _vp(K) if B else None, _vp(T) if B else None, int(nmaxiter),
                                              float(chi2th), int(bool(buse_robust)),
                                              int(bool(bapply_l2_after_robust)), _vp(outl), _vp(ok), _vp(it)))
        off = np.concatenate([[0], np.cumsum(n_pts)])
        return ok[:B].astype(bool), T, [outl[off[b]:off[b + 1]].astype(bool) for b in range(B)], it[:B]

    # -- per-frame epipolar filter (csrc/epipolar.hip) ------------------------------------------------------------------
    def compute5ptEssentialMatrix(self, bvs1, bvs2, nmaxiter, errth, boptimize, bdorandom, fx, fy, seed=0):
        """MultiViewGeometry::compute5ptEssentialMatrix (src/multi_view_geometry.cpp:596-611 -> opengv5ptEssentialMatrix
        :614-697) through ov2_epipolar_filter_batch with B = 1.  bvs1 = keyframe bearings, bvs2 = current-frame bearings.
        returns (success, Rwc (3,3), twc (3,) unit, voutliersidx (sorted int array)): success is the reference's return
        (>= 8 pairs, a model, >= 10 inliers).  bdorandom only selects the seed in the C++ mirror (the caller passes it
        here); boptimize = True (OpenGV's nonlinear refinement) is not built."""
        if boptimize:
            raise NotImplementedError("compute5ptEssentialMatrix: boptimize (OpenGV optimizeModelCoefficients) is not built")
        r = self.compute5ptEssentialMatrix_batch([bvs1], [bvs2], nmaxiter, errth, np.array([[fx, fy, 0., 0.]]), [seed])
        ok = r["status"][0] >= 1
        return bool(ok), r["R"][0], r["t"][0], np.flatnonzero(r["outlier"][0]).astype(np.int32)

    def compute5ptEssentialMatrix_batch(self, bvs1_list, bvs2_list, nmaxiter, errth, K, seeds, gate_kf_list=None,
                                        gate_cur_list=None, R0=None, t0=None):
        """B frames in one launch (ov2_epipolar_filter_batch): RANSAC on each frame's pairs and, where the frame ends with
        status 2, the Sampson gate on its 2D points.  returns dict(status (B,), R (B,3,3), t (B,3), outlier [mask per frame],
        gate_bad [mask per frame], info (B,4))."""
        B = len(bvs1_list)
        n = np.array([len(np.asarray(b).reshape(-1, 3)) for b in bvs1_list], np.int32)
        if any(len(np.asarray(b).reshape(-1, 3)) != k for b, k in zip(bvs2_list, n)):
            raise ValueError("bvs1.size() != bvs2.size()")       # the reference asserts (:622)
        cat = lambda xs, k, dt: (np.concatenate([np.asarray(x, dt).reshape(-1, k) for x in xs]) if B and sum(
            len(np.asarray(x).reshape(-1, k)) for x in xs) else np.zeros((1, k), dt))
        b1, b2 = np.ascontiguousarray(cat(bvs1_list, 3, np.float64)), np.ascontiguousarray(cat(bvs2_list, 3, np.float64))
        ng = np.zeros(B, np.int32) if gate_kf_list is None else \
            np.array([len(np.asarray(g).reshape(-1, 2)) for g in gate_kf_list], np.int32)
        g1 = np.ascontiguousarray(cat(gate_kf_list, 2, np.float32)) if gate_kf_list is not None else np.zeros((1, 2), np.float32)
        g2 = np.ascontiguousarray(cat(gate_cur_list, 2, np.float32)) if gate_cur_list is not None else np.zeros((1, 2), np.float32)
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(B, 4))
        sd = np.ascontiguousarray(np.asarray(seeds, np.uint64).reshape(B))
        R = np.ascontiguousarray(np.zeros((max(B, 1), 9)) if R0 is None else np.array(R0, np.float64).reshape(B, 9))
        t = np.ascontiguousarray(np.zeros((max(B, 1), 3)) if t0 is None else np.array(t0, np.float64).reshape(B, 3))
        outl, gb = np.zeros(max(int(n.sum()), 1), np.uint8), np.zeros(max(int(ng.sum()), 1), np.uint8)
        st, info = np.zeros(max(B, 1), np.int32), np.zeros((max(B, 1), 4), np.int32)
        c = self.ctx
        _check(c.h, c.lib.ov2_epipolar_filter_batch(c.h, B, _vp(n), _vp(b1), _vp(b2), _vp(ng), _vp(g1), _vp(g2), _vp(K),
                                                    int(nmaxiter), float(errth), _vp(sd), _vp(R), _vp(t), _vp(outl),
                                                    _vp(gb), _vp(st), _vp(info)))
        off, goff = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(ng)])
        return dict(status=st[:B], R=R[:B].reshape(B, 3, 3), t=t[:B], info=info[:B],
                    outlier=[outl[off[b]:off[b + 1]].astype(bool) for b in range(B)],
                    gate_bad=[gb[goff[b]:goff[b + 1]].astype(bool) for b in range(B)])

    def compute5ptEssentialMatrix_batch_dev(self, B, d_off, d_bv_kf, d_bv_cur, d_gate_off, d_gate_kf, d_gate_cur, d_K,
                                            nmaxiter, errth, d_seed, d_R, d_t, d_outlier, d_gate_bad, d_status, d_info=None):
        """device-resident, asynchronous form (ov2_epipolar_filter_batch_dev): DeviceArrays in, nothing synchronised."""
        p = lambda a: None if a is None else a.ptr
        c = self.ctx
        _check(c.h, c.lib.ov2_epipolar_filter_batch_dev(c.h, int(B), p(d_off), p(d_bv_kf), p(d_bv_cur), p(d_gate_off),
                                                        p(d_gate_kf), p(d_gate_cur), p(d_K), int(nmaxiter), float(errth),
                                                        p(d_seed), p(d_R), p(d_t), p(d_outlier), p(d_gate_bad),
                                                        p(d_status), p(d_info)))

    # -- mono do_optimize: refinement of the 5-point model on its inliers (csrc/relpose.hip) ------------------------------
    def refine5pt_batch(self, bvs1_list, bvs2_list, K, R0, t0, nmaxiter=10, skip_list=None):
        """B frames in one launch (ov2_relpose_refine_batch): Levenberg-Marquardt on the spherical Sampson cost of
        [R | t], |t| = 1, over the pairs skip_list (the RANSAC outlier masks; None = all pairs) admits.  returns dict(status
        (B,), R (B,3,3), t (B,3) -- the arguments bit for bit where status is 0 --, info (B,2): LM iterations, termination,
        cost (B,2): initial, final)."""
        B = len(bvs1_list)
        n = np.array([len(np.asarray(b).reshape(-1, 3)) for b in bvs1_list], np.int32)
        if any(len(np.asarray(b).reshape(-1, 3)) != k for b, k in zip(bvs2_list, n)):
            raise ValueError("bvs1.size() != bvs2.size()")
        tot = int(n.sum())
        cat = lambda xs, k, dt: (np.concatenate([np.asarray(x, dt).reshape(-1, k) for x in xs]) if tot
                                 else np.zeros((1, k), dt))
        b1, b2 = np.ascontiguousarray(cat(bvs1_list, 3, np.float64)), np.ascontiguousarray(cat(bvs2_list, 3, np.float64))
        sk = None
        if skip_list is not None:
            if any(len(np.asarray(s).reshape(-1)) != k for s, k in zip(skip_list, n)):
                raise ValueError("skip mask size differs from the pair count")
            sk = np.ascontiguousarray(cat(skip_list, 1, np.uint8).ravel())
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(B, 4))
        R = np.ascontiguousarray(np.array(R0, np.float64).reshape(B, 9))
        t = np.ascontiguousarray(np.array(t0, np.float64).reshape(B, 3))
        st, info = np.zeros(max(B, 1), np.int32), np.zeros((max(B, 1), 2), np.int32)
        cost = np.zeros((max(B, 1), 2))
        c = self.ctx
        _check(c.h, c.lib.ov2_relpose_refine_batch(c.h, B, _vp(n), _vp(b1), _vp(b2), None if sk is None else _vp(sk), _vp(K),
                                                   int(nmaxiter), _vp(R), _vp(t), _vp(st), _vp(info), _vp(cost)))
        return dict(status=st[:B], R=R.reshape(B, 3, 3), t=t, info=info[:B], cost=cost[:B])

    def refine5pt_batch_dev(self, B, d_off, d_bv_kf, d_bv_cur, d_skip, d_K, nmaxiter, d_in_status, d_R, d_t, d_status,
                            d_info=None, d_cost=None):
        """device-resident, asynchronous form (ov2_relpose_refine_batch_dev): DeviceArrays in, nothing synchronised.  d_skip,
        d_R, d_t, d_in_status take the d_outlier, d_R, d_t, d_status of compute5ptEssentialMatrix_batch_dev as they are."""
        p = lambda a: None if a is None else a.ptr
        c = self.ctx
        _check(c.h, c.lib.ov2_relpose_refine_batch_dev(c.h, int(B), p(d_off), p(d_bv_kf), p(d_bv_cur), p(d_skip), p(d_K),
                                                       int(nmaxiter), p(d_in_status), p(d_R), p(d_t), p(d_status),
                                                       p(d_info), p(d_cost)))

    def compute5ptEssentialMatrix_opt(self, bvs1, bvs2, nmaxiter, errth, bdorandom, fx, fy, seed=0, nrefine=10):
        """compute5ptEssentialMatrix(..., boptimize = true, ...) of the reference as this project builds it: the RANSAC
        (ov2_epipolar_filter_batch, B = 1), then refine5pt on its inliers (src/multi_view_geometry.cpp:672-681); the
        outlier list stays the RANSAC's.  returns (success, Rwc (3,3), twc (3,) unit, voutliersidx, refined: the
        refinement's status)."""
        K = np.array([[fx, fy, 0., 0.]])
        r = self.compute5ptEssentialMatrix_batch([bvs1], [bvs2], nmaxiter, errth, K, [seed])
        ok = r["status"][0] >= 1
        R, t, refined = r["R"][0], r["t"][0], 0
        if ok:
            q = self.refine5pt_batch([bvs1], [bvs2], K, R, t, nrefine, [r["outlier"][0]])
            R, t, refined = q["R"][0], q["t"][0], int(q["status"][0])
        return bool(ok), R, t, np.flatnonzero(r["outlier"][0]).astype(np.int32), refined

    def dbg_fivept(self, bv1, bv2):
        """the device 5-point solver on n samples (ov2_dbg_fivept): bv1, bv2 (n,5,3) -> E (n,10,3,3), nsol (n,)"""
        bv1, bv2 = np.ascontiguousarray(bv1, np.float64).reshape(-1, 5, 3), np.ascontiguousarray(bv2, np.float64).reshape(-1, 5, 3)
        n = len(bv1)
        E, ns = np.zeros((max(n, 1), 10, 9)), np.zeros(max(n, 1), np.int32)
        c = self.ctx
        _check(c.h, c.lib.ov2_dbg_fivept(c.h, n, _vp(bv1), _vp(bv2), _vp(E), _vp(ns)))
        return E[:n].reshape(n, 10, 3, 3), ns[:n]

    # -- the P3P stage of computePose (csrc/p3p.hip) --------------------------------------------------------------------
    def p3pRansac(self, bvs, vwpts, nmaxiter, errth, boptimize, bdorandom, fx, fy, Twc=None, use_lmeds=True, seed=0):
        """MultiViewGeometry::p3pRansac (src/multi_view_geometry.cpp:144-163 -> opengvP3PLMeds :257-343 / opengvP3PRansac
        :168-254) through ov2_p3p_ransac_batch with B = 1.  returns (success, Twc (7,) [t, qx qy qz qw] -- the argument
        unchanged unless success --, voutliersidx (sorted int array)).  bdorandom only selects the seed in the C++ mirror
        (the caller passes it here); boptimize = True (OpenGV's nonlinear refinement) is not built."""
        if boptimize:
            raise NotImplementedError("p3pRansac: boptimize (OpenGV optimizeModelCoefficients) is not built")
        T0 = np.array([0, 0, 0, 0, 0, 0, 1.]) if Twc is None else np.asarray(Twc, np.float64)
        r = self.p3pRansac_batch([bvs], [vwpts], nmaxiter, errth, np.array([[fx, fy, 0., 0.]]), [seed], use_lmeds, T0[None])
        return bool(r["status"][0]), r["Twc"][0], np.flatnonzero(r["outlier"][0]).astype(np.int32)

    def p3pRansac_batch(self, bvs_list, wpts_list, nmaxiter, errth, K, seeds, use_lmeds=True, Twc0=None):
        """B frames in one call (ov2_p3p_ransac_batch).  returns dict(status (B,), Twc (B,7), outlier [mask per frame],
        info (B,4): counted draws, skipped draws, chosen draw, inliers)."""
        B = len(bvs_list)
        n = np.array([len(np.asarray(b).reshape(-1, 3)) for b in bvs_list], np.int32)
        if any(len(np.asarray(x).reshape(-1, 3)) != k for x, k in zip(wpts_list, n)):
            raise ValueError("bvs.size() != vwpts.size()")       # the reference asserts (:263)
        cat = lambda xs: (np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in xs]) if B and n.sum()
                          else np.zeros((1, 3)))
        bv, X = np.ascontiguousarray(cat(bvs_list)), np.ascontiguousarray(cat(wpts_list))
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(B, 4))
        sd = np.ascontiguousarray(np.asarray(seeds, np.uint64).reshape(B))
        T = np.ascontiguousarray(np.tile([0, 0, 0, 0, 0, 0, 1.], (max(B, 1), 1)) if Twc0 is None
                                 else np.array(Twc0, np.float64).reshape(B, 7))
        outl = np.zeros(max(int(n.sum()), 1), np.uint8)
        st, info = np.zeros(max(B, 1), np.int32), np.zeros((max(B, 1), 4), np.int32)
        c = self.ctx
        _check(c.h, c.lib.ov2_p3p_ransac_batch(c.h, B, _vp(n), _vp(bv), _vp(X), _vp(K), int(nmaxiter), float(errth),
                                               int(bool(use_lmeds)), _vp(sd), _vp(T), _vp(outl), _vp(st), _vp(info)))
        off = np.concatenate([[0], np.cumsum(n)])
        return dict(status=st[:B], Twc=T[:B], info=info[:B], outlier=[outl[off[b]:off[b + 1]].astype(bool) for b in range(B)])

    def p3pRansac_batch_dev(self, B, d_off, d_bvs, d_wpts, d_K, nmaxiter, errth, use_lmeds, d_seed, d_Twc, d_outlier,
                            d_status, d_info=None):
        """device-resident, asynchronous form (ov2_p3p_ransac_batch_dev): DeviceArrays in, nothing synchronised."""
        p = lambda a: None if a is None else a.ptr
        c = self.ctx
        _check(c.h, c.lib.ov2_p3p_ransac_batch_dev(c.h, int(B), p(d_off), p(d_bvs), p(d_wpts), p(d_K), int(nmaxiter),
                                                   float(errth), int(bool(use_lmeds)), p(d_seed), p(d_Twc), p(d_outlier),
                                                   p(d_status), p(d_info)))

    # -- the loop closer's local-map matcher (csrc/match.hip) ----------------------------------------------------------
    def loopMatchToMap_batch(self, inp, fmaxprojerr=10.0, fdistratio=0.3):
        """LoopCloser::matchToMap (src/loop_closer.cpp:586-763) for the B pairs of a loop_match.LoopMatchInput through
        ov2_loop_match_to_map_batch.  returns (match_cand (n_kp,) int32: candidate index within the pair or -1, match_dist)"""
        from . import loop_match
        return loop_match.loopMatchToMap_batch(self.ctx, inp, fmaxprojerr, fdistratio)

    def loopMatchToMap_batch_dev(self, dev_inp, fmaxprojerr=10.0, fdistratio=0.3):
        """device-resident, asynchronous form (ov2_loop_match_to_map_batch_dev) on a loop_match.LoopMatchInputDev: nothing is
        synchronised; dev_inp.get() synchronises and downloads"""
        dev_inp.enqueue(fmaxprojerr, fdistratio)

    def dbg_p3p(self, bv, X):
        """the device P3P solver on n samples (ov2_dbg_p3p): bv, X (n,3,3) -> R (n,4,3,3), t (n,4,3), nsol (n,)"""
        bv, X = np.ascontiguousarray(bv, np.float64).reshape(-1, 3, 3), np.ascontiguousarray(X, np.float64).reshape(-1, 3, 3)
        n = len(bv)
        R, t, ns = np.zeros((max(n, 1), 4, 9)), np.zeros((max(n, 1), 4, 3)), np.zeros(max(n, 1), np.int32)
        c = self.ctx
        _check(c.h, c.lib.ov2_dbg_p3p(c.h, n, _vp(bv), _vp(X), _vp(R), _vp(t), _vp(ns)))
        return R[:n].reshape(n, 4, 3, 3), t[:n], ns[:n]
