#!/usr/bin/env python3
"""bench.py -- tracked frames/s (+ localBA iterations/s) of the MI355X front-end + local-BA hot path.

Contract (driver): python bench.py --gpus N --steps K --warmup W ; for N>1 launched with torch.distributed.run,
one rank per GPU.  W untimed steps, then EXACTLY K timed steps, MAX over ranks, rank 0 prints ONE JSON line.
One bench STEP = `--chunk` (100) frame-batches (= 100 consecutive stereo frames of every sequence), so the driver's
--steps 20 is ~1 s of steady state.  The region starts after barrier + torch.cuda.synchronize(); it ends when the
front-end context's own streams have drained (NOT a device-wide sync, which would also wait for the concurrent
local-BA worker's in-flight batch); the barrier + device sync of the contract follow right after the clock stops.

Workload (BASELINE.json north_star; synthetic because no EuRoC data exists here or on the GPU box):
  synthetic 752x480 stereo streams, `--kps` (2048) keypoints per frame, `--seqs` independent sequences per GPU
  processed in lock-step (one "step" = one new stereo frame of every sequence):
    per frame     : CLAHE + 4-level pyramid + Scharr of the left image  (VisualFrontEnd::preprocessImage)
                    two-stage forward-backward KLT prev->cur            (VisualFrontEnd::kltTracking)
    every KF-th   : right image CLAHE + pyramid, stereo KLT left->right + epipolar gate (Mapper::run /
                    MapManager::stereoMatching: ov2_stereo_matching_dev)
                    [localBA on the keyframe window when the BA path is built: Optimizer::localBA]
  inputs (images, keypoints, priors) are resident in HBM before the timed region; nothing crosses PCIe inside it.
Sequences are independent, so N GPUs = N x seqs sequences, no data-path collective ("scaling": "weak");
RCCL is used only for the end-of-run reduction of {frames, seconds}.

A plain run does only what the headline needs: set-up, warm-up, the K timed steps and the result line.  `--full` adds
the side reports, each outside the timed region: the hipEvent-instrumented pass (`kernels`, `roofline`), the harder
stream, the EuRoC-sized legs and the CPU port baselines.  `--dump-outputs DIR` writes what the timed path computed in
its last step as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H, WIN, NLVL = 752, 480, 9, 3
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=100,
                    help="frame-batches per bench step: one step = `chunk` consecutive stereo frames of every sequence, so that "
                         "the driver's --steps 20 --warmup 5 times a steady-state region of ~1 s instead of 17 ms of launch tail")
    ap.add_argument("--seqs", type=int, default=64, help="independent sequences per GPU (batched per launch); 64 x 2048 keypoints keep the KLT kernels several wave-rounds deep (16: 58k, 64: 97k, 128: 105k, 256: 111k frames/s on one MI355X)")
    ap.add_argument("--kps", type=int, default=2048, help="keypoints per frame (north_star: ~2k)")
    ap.add_argument("--kf-every", type=int, default=6, help="keyframe period (EuRoC sample: 322 KFs / ~2020 frames)")
    ap.add_argument("--frames", type=int, default=8, help="distinct synthetic frames per stream (ping-pong cycle)")
    ap.add_argument("--no-hard-stream", action="store_true", help="skip the harder-stream leg (reported beside the headline, outside the timed region)")
    ap.add_argument("--frame-gap", type=int, default=3, help="stream frames between consecutive bench frames (flow of ~0.6 px per unit)")
    ap.add_argument("--prior-sigma", type=float, default=1.0,
                    help="noise (px) of the motion-model priors; a harder stream (--frame-gap 9 --prior-sigma 3) makes every level "
                         "pass take more LK iterations (the executed mean is reported in config.lk_iterations_per_level_pass)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="budget of EACH cpu_baseline leg (1 thread, N threads)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the N-thread LK leg (0 = every core this process may run on, SURVEY 8d; a 16-thread and a "
                         "1-thread leg are reported beside it)")
    ap.add_argument("--instr-batches", type=int, default=300, help="frame-batches of the instrumented (per-kernel hipEvent) pass")
    ap.add_argument("--ba-kfs", type=int, default=50, help="keyframes in the local-BA window (north_star: ~50)")
    ap.add_argument("--ba-lms", type=int, default=10000, help="landmarks in the local-BA window")
    ap.add_argument("--no-ba", action="store_true", help="front-end only (no concurrent localBA worker)")
    ap.add_argument("--ba-workers", type=int, default=1,
                    help="Estimator threads per GPU (the reference runs one per SLAM instance; each owns a share of the "
                         "sequences and its own high-priority HIP context)")
    ap.add_argument("--fe-priority", default="high", choices=["high", "normal"],
                    help="HIP stream priority of the front-end context: high by default -- the reference's tracking thread is the "
                         "real-time one, the Estimator works on whatever keyframe is newest when it gets to it")
    ap.add_argument("--ba-priority", default="normal", choices=["high", "normal"],
                    help="HIP stream priority of the local-BA workers (high = a pending batch wins the dispatch slots; measured with "
                         "device-resident windows: fe high / ba normal 144.0 k frames/s + 1728 solves/s, fe normal / ba high "
                         "134-136 k + 1810-1836, both high 138.9 k + 1736, both normal 140.8 k + 1760)")
    ap.add_argument("--ba-batch", type=int, default=64, help="most windows one ov2_ba_solve_batch call of a worker takes")
    ap.add_argument("--ba-host-windows", action="store_true",
                    help="legacy leg: ONE window replicated for every sequence, crossing PCIe on every solve (ov2_ba_solve_batch on "
                         "host arrays), solve stage only")
    ap.add_argument("--ba-replicated", action="store_true",
                    help="legacy leg: ONE window replicated for every sequence, resident in HBM, solve stage only (the round-2 "
                         "figure); the default is one DISTINCT device map per sequence with set-up + solve + update per job")
    ap.add_argument("--ba-spread", type=float, default=0.2,
                    help="the sequences' windows draw their keyframes / landmarks within +-spread of --ba-kfs / --ba-lms")
    ap.add_argument("--gen-procs", type=int, default=0, help="processes that generate the synthetic windows (0 = host CPU share, at most 32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-euroc-like", action="store_true",
                    help="skip the EuRoC-sized legs (1 and 8 sequences x 308 keypoints, cell 35, per-frame ceresPnP, 20-KF / 2 k-landmark "
                         "local-BA windows; reported beside the headline, outside the timed region)")
    ap.add_argument("--pnp", action="store_true",
                    help="also run the per-frame pose refinement (ceresPnP, SURVEY 8f row 1) on kps 3D points per frame, "
                         "device-resident; off by default: the BASELINE metric is the tracking path")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--mapper-ctx", type=int, default=0,
                    help="1: the keyframe's right-image pyramid + stereo KLT run on a second context (the reference's mapper "
                         "thread, src/mapper.cpp:76-97), overlapping the front-end's next frames")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (= RCCL over xGMI) for the real multi-GPU run; gloo rehearses the N > 1 control flow with "
                         "several ranks sharing one GPU")
    ap.add_argument("--full", action="store_true",
                    help="also run the side reports after the timed region: instrumented per-kernel pass + roofline, harder "
                         "stream, EuRoC-sized legs, CPU port baselines (each still switchable off with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                         "(float32 / float64, at most 64 MB in all; rank 0's sequences)")
    return ap.parse_args()


# --------------------------------------------------------------------------------------------------
def lk_bytes(work_words):
    """one level pass = 500 B template fetch, one LK iteration = 100 B of J."""
    w = np.asarray(work_words, np.uint32)
    return 500.0 * float((w >> 16).sum()) + 100.0 * float((w & 0xffff).sum())


def lk_ops(work_words):
    """one level pass = 2.7 kop of template set-up, one LK iteration = 1.0 kop (81 px x (bilinear 10 + 2 MAC))."""
    w = np.asarray(work_words, np.uint32)
    return 2700.0 * float((w >> 16).sum()) + 1000.0 * float((w & 0xffff).sum())


VALU_PEAK_TOPS = 78.6   # MI355X vector peak in lane-instructions/s: 157.3 TFLOP/s fp32 / 2 (an FMA counts twice)


def pyr_level_bytes(w, h, nlevels):
    """per level_kernel launch of a build: read level l (u8), write level l+1 (u8).  The Scharr planes (4 B/px) are no
    longer part of a build: the 9x9 tracking kernels derive them from the image windows, and the planes are only written
    when a consumer asks for them (ov2_pyr_need_grad)."""
    out, cw, ch = [], w, h
    for l in range(nlevels - 1):
        nw, nh = (cw + 1) // 2, (ch + 1) // 2
        out.append(cw * ch + nw * nh)
        cw, ch = nw, nh
    return out


class Workload:
    """everything resident in HBM: per cycle position c, the left/right image batches, keypoints, priors."""

    def __init__(self, ctx, fe, synth, seqs, kps, nframes, seed, gap=3, prior_sigma=1.0, det_cell=None):
        self.ctx, self.fe, self.B, self.N = ctx, fe, seqs, kps
        self.gap, self.prior_sigma = gap, prior_sigma
        S = synth.StereoStream(seed=seed)
        F = nframes
        left = [S.left(gap * t) for t in range(F)]    # `gap` stream-frames apart: flow of 1-2 px per step at gap 3
        right = [S.right(gap * t) for t in range(F)]
        order = list(range(F)) + list(range(F - 2, 0, -1))   # ping-pong so consecutive frames are adjacent
        self.L = L = len(order)
        self.trk = fe.FeatureTracker(ctx, 30, 0.01)
        base = synth.grid_keypoints(kps, seed=seed + 7)
        self.left, self.right, self.kps, self.pri, self.has = [], [], [], [], []
        self.has_host = []
        self.st_pri, self.st_has = [], []
        for c in range(L):
            il, ir = fe.Images(ctx, seqs, W, H), fe.Images(ctx, seqs, W, H)
            k_all, p_all, h_all, sp_all, sh_all = [], [], [], [], []
            for b in range(seqs):
                cur = order[(c + 3 * b) % L]
                prv = order[(c - 1 + 3 * b) % L]
                il.upload(b, left[cur])
                ir.upload(b, right[cur])
                # keypoints live in the PREVIOUS frame; the prior is the motion-model prediction in the current one
                gt = S.flow(gap * prv, gap * cur, base)
                pri, has = synth.make_priors(base, gt, sigma=prior_sigma, seed=seed + 11 + 31 * c + b)
                spri, shas = synth.make_priors(base, S.stereo_gt(base), sigma=prior_sigma, seed=seed + 13 + 31 * c + b)
                k_all.append(base); p_all.append(pri); h_all.append(has); sp_all.append(spri); sh_all.append(shas)
            self.left.append(il); self.right.append(ir)
            self.kps.append(ctx.to_device(np.concatenate(k_all)))
            self.pri.append(ctx.to_device(np.concatenate(p_all)))
            self.has.append(ctx.to_device(np.concatenate(h_all)))
            self.has_host.append(np.concatenate(h_all).astype(bool))
            self.st_pri.append(ctx.to_device(np.concatenate(sp_all)))
            self.st_has.append(ctx.to_device(np.concatenate(sh_all)))
        n = seqs * kps
        self.n = n
        self.img_idx = ctx.to_device(np.repeat(np.arange(seqs, dtype=np.int32), kps))
        self.out_xy = ctx.empty((n, 2), np.float32)
        self.out_st = ctx.empty((n,), np.uint8)
        self.p3p = ctx.empty((seqs,), np.int32)
        self.work = ctx.empty((2 * n,), np.uint32)
        self.prev = None
        self.step_no = 0
        self.host_frames = (left, right, order, base, S)
        # keyframe creation (MapManager::extractKeypoints -> detectSingleScale): cell size such that the grid holds
        # ~kps cells (nmaxdist of the YAML plays this role: 35 px <-> 308 kps); 85 % of the cells hold a tracked kp
        self.det_cell = det_cell or max(8, int(np.sqrt(W * H / float(kps))))
        rng = np.random.default_rng(seed + 5)
        self.det_cur = [base[rng.uniform(size=len(base)) < 0.85] for _ in range(seqs)]
        self.det_thresh = np.full(seqs, 0.001, np.float64)
        self.n_detected = 0
        # keyframe detection runs device-resident (ov2_detect_grid_batch_dev): thresholds, existing keypoints, counts and
        # new corners live in HBM, so a keyframe costs no host synchronisation
        self.det_ncur = int(sum(len(c) for c in self.det_cur))
        self.d_det_cur = ctx.to_device(np.ascontiguousarray(np.concatenate(self.det_cur), np.float32))
        self.d_det_img = ctx.to_device(np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(self.det_cur)]))
        self.det_cap = max(1, (W // self.det_cell) * (H // self.det_cell)) * 2
        self.d_det_thresh = ctx.to_device(self.det_thresh)
        self.d_det_out = ctx.empty((seqs, self.det_cap, 2), np.float32)
        self.d_det_nout = ctx.empty((seqs,), np.int32)

    detect = True
    pnp = None
    mctx = None

    def enable_mapper_ctx(self, device):
        """Mapper::run's share of a keyframe (right pyramid + stereoMatching) on its own context / streams"""
        fe = self.fe
        self.mctx = fe.Context(device)
        self.mtrk = fe.FeatureTracker(self.mctx, 30, 0.01)
        self.m_out_xy = self.mctx.empty((self.n, 2), np.float32)
        self.m_out_st = self.mctx.empty((self.n,), np.uint8)
        self.m_p3p = self.mctx.empty((self.B,), np.int32)

    def enable_pnp(self, seed):
        """per-frame computePose stand-in: one synthetic pose-refinement problem per sequence (kps points, 10 % outliers,
        perturbed initial pose), device-resident; every step re-solves it from the same initial pose."""
        from ov2slam_amd import synth_ba
        from ov2slam_amd.multi_view_geometry import MultiViewGeometry
        ctx, B, N = self.ctx, self.B, self.N
        fr = [synth_ba.make_pnp(N, seed=seed + 7 * b) for b in range(B)]
        self.pnp = dict(mvg=MultiViewGeometry(ctx),
                        off=ctx.to_device(np.arange(B + 1, dtype=np.int32) * N),
                        unpx=ctx.to_device(np.concatenate([f["unpx"] for f in fr])),
                        wpts=ctx.to_device(np.concatenate([f["wpts"] for f in fr])),
                        K=ctx.to_device(np.stack([f["K"] for f in fr])),
                        T0=ctx.to_device(np.stack([f["Twc0"] for f in fr])), T=ctx.empty((B, 7), np.float64),
                        outl=ctx.empty((B * N,), np.uint8), rem=ctx.empty((B * N,), np.uint8),
                        ok=ctx.empty((B,), np.int32))

    def step(self, kf_every, want_work=False):
        fe, ctx, c = self.fe, self.ctx, self.step_no % self.L
        cur = fe.preprocess_images(ctx, self.left[c], True, 3.0, WIN, NLVL)           # 2.FE_TM_preprocessImage
        work = self.work if want_work else None
        if self.prev is not None:                                                    # 2.FE_TM_KLT-Tracking
            self.trk.kltTracking_dev(self.prev, cur, WIN, NLVL, 30.0, 0.5, self.kps[c], self.pri[c], self.has[c],
                                     self.out_xy, self.out_st, self.n, self.img_idx, self.p3p, work)
            self.prev.release()
            if self.pnp:                                                              # 2.FE_TM_computePose (ceresPnP)
                q = self.pnp
                q["T"].copy_from(q["T0"])
                q["mvg"].ceresPnP_batch_dev(self.B, q["off"], q["unpx"], q["wpts"], None, q["K"], q["T"], 5, 5.9915, True,
                                            True, q["outl"], q["rem"], q["ok"])
        self.prev = cur
        is_kf = (self.step_no % kf_every) == 0
        if is_kf and self.mctx is not None:                                          # 1.KF_stereoMatching on the mapper's context
            kfpyr = cur.retain()                                                      # Keyframe keeps the pyramid (src/ov2slam.cpp:175-180)
            rp = fe.preprocess_images(self.mctx, self.right[c], True, 3.0, WIN, NLVL)
            self.mtrk.stereoMatching_dev(kfpyr, rp, WIN, NLVL, 30.0, 0.5, self.kps[c], self.st_pri[c], self.st_has[c],
                                         self.m_out_xy, self.m_out_st, self.n, self.img_idx, None, True, None)
            rp.release()
            kfpyr.release_from(self.mctx)
        elif is_kf:                                                                  # 1.KF_stereoMatching
            rp = fe.preprocess_images(ctx, self.right[c], True, 3.0, WIN, NLVL)
            self.trk.stereoMatching_dev(cur, rp, WIN, NLVL, 30.0, 0.5, self.kps[c], self.st_pri[c], self.st_has[c],
                                        self.out_xy, self.out_st, self.n, self.img_idx, None, True, None)
            rp.release()
            if self.detect:                                                           # 1.FE_createKeyframe (detector)
                fe.detect_grid_batch_dev(ctx, cur, self.det_cell, 1, self.d_det_thresh, self.det_ncur, self.d_det_cur,
                                         self.d_det_img, None, self.d_det_nout, self.d_det_out, self.det_cap)
        self.step_no += 1
        return is_kf


class BaPipeline:
    """the Estimator threads of the reference (src/estimator.cpp:32-98), one SLAM instance per sequence, each with its OWN
    map: a device-resident ov2_map holding a distinct synthetic window (its own keyframe / landmark counts, outlier rate,
    initial error).  A keyframe job is the WHOLE of Optimizer::localBA on that map: set-up (covisibility walk -> flat
    problem, src/optimizer.cpp:43-430) -> solve (:439-735) -> update (:741-882), batched over every sequence that has a
    keyframe pending (ov2_map_local_ba_setup_batch -> ov2_ba_solve_batch_dev -> ov2_map_local_ba_update_batch).  Every job
    starts from the map's saved state (the stand-in for the mapper having just added the keyframe).  Native thread(s) of
    libov2host.so on their own HIP context(s)."""

    def __init__(self, fe, device, windows, specs, workers=1, max_batch=64, high_priority=False):
        from ov2slam_amd import device_map as DM, host_map
        self.DM, self.windows, self.specs = DM, windows, specs
        seqs = len(windows)
        workers = max(1, min(workers, seqs))
        share = [seqs // workers + (1 if k < seqs % workers else 0) for k in range(workers)]
        self.ctxs, self.maps, self.ws = [], [], []
        i = 0
        for k in range(workers):
            c = fe.Context(device, high_priority=high_priority)
            ms = [DM.DeviceMap.from_problem(c, P, isobs="newest") for P in windows[i:i + share[k]]]
            for m in ms:
                m.save_state()
            i += share[k]
            self.ctxs.append(c); self.maps.append(ms)
        # the flat problems the set-up makes of these maps (sizes for the report; also the first use of every block)
        self.flat = []
        for c, ms in zip(self.ctxs, self.maps):
            for v in DM.setup_batch(c, ms, calib_l=windows[0].calib_l):
                self.flat.append(dict(aborted=bool(v.aborted), poses=int(v.n_pose), landmarks=int(v.n_lm), residual_blocks=int(v.n_res)))
            DM.restore_state_batch(c, ms)
            c.synchronize()
        for c, ms in zip(self.ctxs, self.maps):
            self.ws.append(host_map.EstimatorPipeline(c, ms, windows[0], max_batch=max_batch))
        for w in self.ws:
            w.submit_all()                        # warm-up (arenas, code objects); not counted
        self.solves = self.iters = self.dropped = self.submitted = self.batches = 0
        self.busy_s = 0.0
        self.tot = {}
        self.mode = (f"{workers} native worker thread(s), each on its own {'high' if high_priority else 'normal'}-priority HIP "
                     f"context, concurrent with the front-end; every sequence owns a device-resident map (ov2_map) with a DISTINCT "
                     f"window; a keyframe job = set-up + solve + update of Optimizer::localBA on that map; a worker serves all its "
                     f"sequences that have a keyframe pending in one batch (<= {max_batch}): ov2_map_local_ba_setup_batch -> "
                     f"ov2_ba_solve_batch_dev -> ov2_map_local_ba_update_batch; robust solve (<=5 it) + L2 (<=10 it); a newer "
                     f"keyframe of a sequence replaces its pending one (src/estimator.cpp:185-210)")

    def submit_all(self):
        for w in self.ws:
            w.submit_all()

    def set_counting(self, on):
        for w in self.ws:
            w.set_counting(on)

    def refresh(self):
        tot = None
        for w in self.ws:
            st = w.stats()
            if st["last_status"] != 0:
                raise RuntimeError(f"the local-BA pipeline failed in the worker (status {st['last_status']})")
            if tot is None:
                tot = st
            else:
                for k, v in st.items():
                    tot[k] = [x + y for x, y in zip(tot[k], v)] if isinstance(v, list) else tot[k] + v
        self.solves, self.iters, self.dropped = tot["solves"], tot["iters"], tot["dropped"]
        self.submitted, self.busy_s, self.batches = tot["submitted"], tot["busy_s"] / len(self.ws), tot["batches"]
        self.tot = tot
        return tot

    def stop(self):
        for w in self.ws:
            w.close()

    def flat_problems(self, k):
        """the first k flat problems as host BaProblems (for the CPU leg); the workers must have been stopped"""
        from ov2slam_amd.ba_types import BaProblem
        DM, out = self.DM, []
        c, ms = self.ctxs[0], self.maps[0][:k]
        DM.restore_state_batch(c, ms)
        P0 = self.windows[0]
        for v in DM.setup_batch(c, ms, calib_l=P0.calib_l):
            f = DM.fetch_view(c, v, True)
            if f["aborted"]:
                continue
            out.append(BaProblem(P0.calib_l, P0.calib_r, P0.T_rl, 1, f["pose"], f["pose_const"], f["lm"],
                                 np.searchsorted(f["pose_kfid"], f["lm_anchor_kfid"]).astype(np.int32), f["lm_anchor_uv"],
                                 f["res_type"], np.searchsorted(f["pose_kfid"], f["res_kfid"]).astype(np.int32),
                                 np.searchsorted(f["lm_lmid"], f["res_lmid"]).astype(np.int32), f["res_uv"], f["res_sigma"]))
        return out


class BaWorker:
    """the Estimator thread of the reference (src/estimator.cpp:32-98): runs Optimizer::localBA on the newest pending
    keyframe of any sequence, on its own high-priority HIP context/stream, concurrently with the front-end; a keyframe
    that arrives while its sequence still has one pending replaces it (src/estimator.cpp:185-210 keeps only the
    newest).  The loop is a NATIVE thread of libov2host.so (ov2slam_amd/host/ov2_host_capi.cpp): a Python thread here
    fought the front-end loop for the interpreter lock and made the frames/s depend on the host's load."""

    def __init__(self, device, seqs, n_kf, n_lm, seed, workers=1, max_batch=64, high_priority=True, device_resident=True):
        """legacy legs (--ba-replicated / --ba-host-windows): one window for every sequence, solve stage only"""
        from ov2slam_amd import host_map, synth_ba
        self.P0 = synth_ba.make_window(n_kf, n_lm, inv_depth=True, seed=seed, max_obs=7)
        workers = max(1, min(workers, seqs))
        share = [seqs // workers + (1 if k < seqs % workers else 0) for k in range(workers)]
        self.ws = [host_map.EstimatorWorker(device, self.P0, share[k], max_batch=max_batch, high_priority=high_priority,
                                            device_resident=device_resident)
                   for k in range(workers)]
        for w in self.ws:
            w.submit_all()                        # warm-up (allocations, code objects); not counted
        self.solves = self.iters = self.dropped = self.submitted = 0
        self.busy_s = 0.0
        self.batches = 0
        self.mode = (f"{workers} native worker thread(s), each on its own {'high' if high_priority else 'normal'}-priority HIP stream, concurrent with the front-end; a "
                     f"worker solves the windows of all its sequences that have a keyframe pending in ONE "
                     f"{'ov2_ba_solve_batch_dev call on windows resident in HBM' if device_resident else 'ov2_ba_solve_batch call on host windows (PCIe-inclusive)'} "
                     f"(<= {max_batch} windows; reference: one Estimator thread per SLAM instance, src/estimator.cpp:32-98); "
                     "robust solve (<=5 it) + L2 (<=10 it); a newer keyframe of a sequence replaces its pending one")

    def submit_all(self):
        for w in self.ws:
            w.submit_all()

    def set_counting(self, on):
        for w in self.ws:
            w.set_counting(on)

    def refresh(self):
        tot = dict(solves=0, iters=0, dropped=0, submitted=0, busy_s=0.0, batches=0)
        for w in self.ws:
            st = w.stats()
            if st["last_status"] != 0:
                raise RuntimeError(f"ov2_ba_solve failed in the worker (status {st['last_status']})")
            for k in tot:
                tot[k] += st[k]
        self.solves, self.iters, self.dropped = tot["solves"], tot["iters"], tot["dropped"]
        self.submitted, self.busy_s = tot["submitted"], tot["busy_s"] / len(self.ws)
        self.batches = tot["batches"]
        return tot

    def stop(self):
        for w in self.ws:
            w.close()


def cpu_baseline(workload, kf_every, budget_s, threads=1):
    """the oracle (a C port of the OpenCV path) timed on this host on a bounded sample of the SAME workload (one
    sequence); `threads` > 1 splits the points of every LK call over a persistent thread pool, as OpenCV's
    parallel_for_ does (CLAHE + pyramid stay on one thread).  Reported beside the GPU number, never shipped."""
    from oracle import oracle_py as O
    O.set_num_threads(threads)
    left, right, order, base, S = workload.host_frames
    from ov2slam_amd import synth
    L = len(order)
    # priors of every cycle position, made before the clock starts (numpy; not part of the path)
    tpri, spri = [], []
    for s in range(L):
        cur_i, prv_i = order[s % L], order[(s - 1) % L]
        tpri.append(synth.make_priors(base, S.flow(workload.gap * prv_i, workload.gap * cur_i, base), sigma=workload.prior_sigma, seed=1 + s))
        spri.append(synth.make_priors(base, S.stereo_gt(base), sigma=workload.prior_sigma, seed=2 + s))
    t0 = time.perf_counter()
    prev, frames, s = None, 0, 0
    while True:
        cur_i = order[s % L]
        cur = O.Pyramid(O.clahe(left[cur_i], 3.0, 15, 9), WIN, NLVL)
        if prev is not None:
            pri, has = tpri[s % L]
            O.klt_tracking_frame(prev, cur, base, pri, has, WIN, NLVL, 30.0, 0.5, 30, 0.01)
        if s % kf_every == 0:
            rp = O.Pyramid(O.clahe(right[cur_i], 3.0, 15, 9), WIN, NLVL)
            pri, has = spri[s % L]
            O.stereo_matching(cur, rp, base, pri, has, WIN, NLVL, 30.0, 0.5, 30, 0.01, rectified=True)
        prev = cur
        frames += 1
        s += 1
        el = time.perf_counter() - t0
        if el > budget_s and frames >= 2 * kf_every:
            break
    O.set_num_threads(1)
    return frames / el, frames, el


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(path, wl, ba):
    """--dump-outputs: the arrays the timed path hands its caller after its last step, as path/<name>.npy.
      frame_xy / frame_status / frame_p3p_req  the tracking buffers of the last frame (kltTracking_dev; on a keyframe the
                                               stereo matching of the same frame is their last writer)
      kf_stereo_xy / kf_stereo_status          stereo matching of the last keyframe, when it runs on the mapper context
      kf_corners_xy / kf_corner_count /        grid detector of the last keyframe (rows past a sequence's count are zero)
      kf_detect_threshold
      pnp_pose / pnp_outlier / pnp_ok          per-frame ceresPnP of the last frame (--pnp)
      ba_kf_pose / ba_kf_state / ba_lm_xyz /   every sequence's device map after its last local-BA job (set-up + solve +
      ba_lm_state / ba_map_sizes               update from the saved state), maps concatenated in sequence order
    Every array is float32 or float64.  Past DUMP_CAP_BYTES in all, the long arrays keep a fixed seeded sample of their
    rows (sorted; the row indices are written as <name>_rows.npy)."""
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    out = {"frame_xy": f32(wl.out_xy.get()), "frame_status": f32(wl.out_st.get()), "frame_p3p_req": f32(wl.p3p.get())}
    if wl.mctx is not None:
        out["kf_stereo_xy"], out["kf_stereo_status"] = f32(wl.m_out_xy.get()), f32(wl.m_out_st.get())
    elif wl.detect:
        n = wl.d_det_nout.get().astype(np.int64)
        xy = wl.d_det_out.get()
        xy[np.arange(xy.shape[1])[None, :] >= n[:, None]] = 0.0
        out["kf_corners_xy"], out["kf_corner_count"] = f32(xy), f32(n)
        out["kf_detect_threshold"] = np.ascontiguousarray(wl.d_det_thresh.get(), np.float64)
    if wl.pnp:
        q = wl.pnp
        out["pnp_pose"], out["pnp_outlier"], out["pnp_ok"] = q["T"].get(), f32(q["outl"].get()), f32(q["ok"].get())
    if isinstance(ba, BaPipeline):
        tabs = [m.download() for ms in ba.maps for m in ms]
        out["ba_kf_pose"] = np.concatenate([t["kf_pose"] for t in tabs])
        out["ba_kf_state"] = f32(np.concatenate([t["kf_state"] for t in tabs]))
        out["ba_lm_xyz"] = np.concatenate([t["lm_xyz"] for t in tabs])
        out["ba_lm_state"] = f32(np.concatenate([t["lm_state"] for t in tabs]))
        out["ba_map_sizes"] = np.asarray([[len(t["kf_pose"]), len(t["lm_xyz"])] for t in tabs], np.float64)
    if sum(v.nbytes for v in out.values()) > DUMP_CAP_BYTES:
        long_ = sorted(k for k, v in out.items() if len(v) > 4096)
        short = sum(out[k].nbytes for k in out if k not in long_)
        # a sampled row costs its own bytes + 8 for its index
        keep = (0.95 * DUMP_CAP_BYTES - short) / sum(out[k].nbytes + 8 * len(out[k]) for k in long_)
        rng = np.random.default_rng(12345)
        for k in long_:
            v = out[k]
            rows = np.sort(rng.choice(len(v), max(1, int(keep * len(v))), replace=False))
            out[k], out[k + "_rows"] = np.ascontiguousarray(v[rows]), rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, v in out.items():
        assert v.dtype in (np.float32, np.float64), k
        np.save(os.path.join(path, k + ".npy"), v)
    return sorted(out)


def main():
    a = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    legacy_ba = a.ba_replicated or a.ba_host_windows
    windows = specs = None
    if not a.no_ba and not legacy_ba:
        # one DISTINCT local-BA window per sequence (numpy; spawned worker processes, made before this process touches the GPU)
        from ov2slam_amd import synth_ba
        try:
            share = len(os.sched_getaffinity(0))
        except Exception:
            share = os.cpu_count() or 1
        # at most 16: the affinity mask can show far more cores than the process's CPU share (the windows do not depend on it)
        procs = a.gen_procs if a.gen_procs > 0 else max(1, min(16, share // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world)))))
        specs = synth_ba.sequence_window_specs(a.seqs, seed=20211 + 100003 * rank, n_kf=a.ba_kfs, n_lm=a.ba_lms, spread=a.ba_spread)
        t_gen = time.perf_counter()
        windows = synth_ba.make_windows_parallel(specs, procs)
        t_gen = time.perf_counter() - t_gen
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    if a.dist_backend == "gloo":
        local = local % torch.cuda.device_count()   # rehearsal: ranks share the GPUs that exist
    torch.cuda.set_device(local)
    from ov2slam_amd import dist_util
    dist_util.init_from_env(a.dist_backend, torch.device("cuda", local))   # nccl == RCCL on ROCm

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    from ov2slam_amd import frontend as fe, synth
    ctx = fe.Context(local, high_priority=a.fe_priority == "high")
    wl = Workload(ctx, fe, synth, a.seqs, a.kps, a.frames, seed=synth.SEED_IMG + 101 * rank, gap=a.frame_gap, prior_sigma=a.prior_sigma)

    if a.mapper_ctx:
        wl.enable_mapper_ctx(local)
    if a.pnp:
        wl.enable_pnp(seed=777 + rank)
    ba = None
    if not a.no_ba and legacy_ba:
        ba = BaWorker(local, a.seqs, a.ba_kfs, a.ba_lms, seed=20211 + rank, workers=a.ba_workers, max_batch=a.ba_batch,
                      high_priority=a.ba_priority == "high", device_resident=not a.ba_host_windows)
    elif not a.no_ba:
        ba = BaPipeline(fe, local, windows, specs, workers=a.ba_workers, max_batch=a.ba_batch, high_priority=a.ba_priority == "high")
    def run_step():
        """one bench step = a.chunk frame-batches; returns the number of keyframe batches it held"""
        k = 0
        for _ in range(a.chunk):
            kf = wl.step(a.kf_every)
            k += kf
            if kf and ba:
                ba.submit_all()                 # Mapper::run -> Estimator::addNewKf
        return k

    for _ in range(a.warmup):
        run_step()
    ctx.synchronize()
    barrier()
    if ba:
        ba.set_counting(True)
    t0 = time.perf_counter()
    ctx.timer_start()
    nkf = 0
    for _ in range(a.steps):
        nkf += run_step()
    t_enq = time.perf_counter() - t0   # host time to enqueue the K steps
    gpu_ms = ctx.timer_stop()          # synchronises the ctx main stream
    ctx.synchronize()                  # ... and the pyramid stream: every launch of the K steps has completed
    if wl.mctx is not None:
        wl.mctx.synchronize()
    el = time.perf_counter() - t0
    if ba:
        ba.set_counting(False)         # solves that complete after this instant do not count
        ba.refresh()
        ba.stop()                      # joins the worker threads: their in-flight batch runs to its end
    barrier()                          # the contract's closing barrier + device sync, outside the clock (it would wait for
                                       # the BA worker's in-flight batch, which is not front-end work)
    el_closed = time.perf_counter() - t0   # ... the same interval closed by the device-wide sync (both conventions are reported)
    nbatches = a.steps * a.chunk

    # {frames, BA LM iterations, BA solves, BA jobs submitted, dropped}: the end-of-run reduction over RCCL
    el_max, cnt = dist_util.aggregate(el, [nbatches * a.seqs, ba.iters if ba else 0, ba.solves if ba else 0,
                                           ba.submitted if ba else 0, ba.dropped if ba else 0],
                                       device="cuda" if a.dist_backend == "nccl" else "cpu")
    frames_all, ba_iters_all, ba_solves_all, ba_sub_all, ba_drop_all = cnt

    out = {
        "metric": "tracked_frames_per_sec", "value": frames_all / el_max, "unit": "frames/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * el_max / a.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8/s16 fixed-point + f32",
        "data": "synthetic",
        "config": {"workload": "synthetic 752x480 stereo streams, CLAHE + 4-level pyramid + 2-stage fwd-bwd KLT "
                               f"(win 9, 30 it, eps 0.01) on {a.kps} kps/frame; every {a.kf_every}th frame is a keyframe: "
                               f"right-image pyramid + stereo KLT + grid detector (min-eig, cell {wl.det_cell} px) + "
                               f"cornerSubPix; {a.seqs} sequences per GPU in lock-step; one bench step = {a.chunk} "
                               f"consecutive frames of every sequence ({a.chunk * a.seqs} frames per GPU)"
                               + ("; per-frame ceresPnP pose refinement on the same stream" if a.pnp else ""),
                   "sequences_per_gpu": a.seqs, "keypoints_per_frame": a.kps, "kf_every": a.kf_every,
                   "frame_batches_per_step": a.chunk, "frames_per_step_per_gpu": a.chunk * a.seqs,
                   "image": [W, H], "parallelism": f"replicas x{world} (one batch of sequences per GPU)"},
        "ms_per_frame_batch": 1e3 * el_max / nbatches,
        "gpu_stream_ms_per_frame_batch": gpu_ms / nbatches,
        "host_enqueue_ms_per_frame_batch": 1e3 * t_enq / nbatches,
        "keyframe_batches_per_frame_batch": nkf / nbatches,
        "timed_region_s": el_max,
        "with_closing_device_sync": {"seconds": el_closed, "frames_per_sec": nbatches * a.seqs * world / el_closed if world == 1 else None,
                                     "note": "the same K steps with the contract's barrier + device-wide synchronisation inside the clock: it "
                                             "also waits for the local-BA worker's in-flight batch (whose solves are NOT counted) to drain"},
    }
    if ba and legacy_ba:
        out["local_ba"] = {"metric": "localBA_LM_iterations_per_sec", "value": ba_iters_all / el_max, "unit": "iters/s",
                           "solves_per_sec": ba_solves_all / el_max, "solves": ba_solves_all,
                           "measured_over": "timed region (solves that started and completed inside it, concurrent with the "
                                            "front-end); LEGACY leg: one window replicated for every sequence, solve stage only",
                           "keyframe_jobs_submitted": ba_sub_all, "jobs_replaced_by_newer_kf": ba_drop_all,
                           "replaced_fraction": (ba_drop_all / ba_sub_all) if ba_sub_all else 0.0,
                           "window": {"keyframes": a.ba_kfs, "landmarks": a.ba_lms, "residual_blocks": int(ba.P0.n_res),
                                      "parametrisation": "anchored inverse depth (buse_inv_depth: 1)"},
                           "workers_per_gpu": len(ba.ws), "batches": ba.batches,
                           "windows_per_batch": (ba.solves / ba.batches) if ba.batches else 0.0,
                           "mode": ba.mode,
                           "worker_busy_frac": (ba.busy_s / el) if el > 0 else 0.0}
        # one LM iteration touches every residual block once (32 B record + 16 B residual + 208 B jacobian for
        # the inverse-depth functors), S twice and the parameters once
        n_free = int((ba.P0.pose_const == 0).sum())
        it_bytes = ba.P0.n_res * 256.0 + 2.0 * (6 * n_free) ** 2 * 8.0 + (7 * len(ba.P0.pose) + len(ba.P0.lm)) * 8.0
        lb = out["local_ba"]
        lb["roofline"] = {"bound": "hbm", "alg_bytes_per_lm_iteration": it_bytes, "achieved": lb["value"] * it_bytes / 1e9,
                          "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": lb["value"] * it_bytes / 1e9 / HBM_PEAK_GBS,
                          "note": "LM iterations/s of all windows x algorithmic bytes of one iteration, concurrent with the front-end"}
        out["config"]["workload"] += f"; localBA on a {a.ba_kfs}-KF / {a.ba_lms}-landmark window per keyframe job"
    elif ba:
        T = ba.tot
        ok = [f for f in ba.flat if not f["aborted"]]
        rng3 = lambda key: [int(min(f[key] for f in ok)), float(np.mean([f[key] for f in ok])), int(max(f[key] for f in ok))]
        nb = max(T["batches"], 1)
        out["local_ba"] = {"metric": "localBA_LM_iterations_per_sec", "value": ba_iters_all / el_max, "unit": "iters/s",
                           "solves_per_sec": ba_solves_all / el_max, "solves": ba_solves_all,
                           "what_a_solve_is": "distinct windows, set-up + solve + update: one whole Optimizer::localBA on the "
                                              "sequence's own device-resident map (src/optimizer.cpp:43-430 + 439-735 + 741-882)",
                           "measured_over": "timed region (jobs that started and completed inside it, concurrent with the front-end)",
                           "keyframe_jobs_submitted": ba_sub_all, "jobs_replaced_by_newer_kf": ba_drop_all,
                           "replaced_fraction": (ba_drop_all / ba_sub_all) if ba_sub_all else 0.0,
                           "windows": {"distinct": len(ba.flat), "aborted_setups": len(ba.flat) - len(ok),
                                       "nominal": {"keyframes": a.ba_kfs, "landmarks": a.ba_lms, "spread": a.ba_spread},
                                       "poses_min_mean_max": rng3("poses"), "landmarks_min_mean_max": rng3("landmarks"),
                                       "residual_blocks_min_mean_max": rng3("residual_blocks"),
                                       "outlier_fraction_min_max": [min(sp["outlier_frac"] for sp in specs), max(sp["outlier_frac"] for sp in specs)],
                                       "parametrisation": "anchored inverse depth (buse_inv_depth: 1)",
                                       "generated_in_s": t_gen},
                           "lm_iterations_per_window": {"robust_histogram_0_to_7": T["hist_robust"], "l2_histogram_0_to_15": T["hist_l2"],
                                                        "mean": (T["iters"] / T["solves"]) if T["solves"] else 0.0,
                                                        "slowest_window_of_a_batch_mean": T["slowest_sum"] / nb,
                                                        "note": "a batch runs as long as its slowest window: robust pass <= 5, L2 pass <= 10"},
                           "workers_per_gpu": len(ba.ws), "batches": ba.batches,
                           "windows_per_batch": (ba.solves / ba.batches) if ba.batches else 0.0,
                           "ms_per_batch": {"setup_incl_state_restore": 1e3 * T["setup_s"] / nb, "solve": 1e3 * T["solve_s"] / nb,
                                            "update_incl_final_sync": 1e3 * T["update_s"] / nb,
                                            "setup_per_window": 1e3 * T["setup_s"] / max(T["solves"], 1)},
                           "mode": ba.mode,
                           "worker_busy_frac": (ba.busy_s / el) if el > 0 else 0.0}
        # one LM iteration touches every residual block once (32 B record + 16 B residual + 208 B jacobian for
        # the inverse-depth functors), S twice and the parameters once; summed over the windows actually iterated
        mean_free = float(np.mean([f["poses"] - 1 for f in ok])) if ok else 0.0
        mean_par = float(np.mean([7 * f["poses"] + f["landmarks"] for f in ok])) * 8.0 if ok else 0.0
        bytes_all = T["iter_blocks"] * 256.0 + T["iters"] * (2.0 * (6 * mean_free) ** 2 * 8.0 + mean_par)
        lb = out["local_ba"]
        lb["roofline"] = {"bound": "hbm", "alg_bytes_total": bytes_all, "achieved": bytes_all / el / 1e9, "peak": HBM_PEAK_GBS,
                          "unit": "GB/s", "frac": bytes_all / el / 1e9 / HBM_PEAK_GBS,
                          "note": "sum over the solved windows of LM iterations x algorithmic bytes of one iteration of THAT window "
                                  "(256 B per residual block + S twice + parameters), over the timed region, concurrent with the front-end"}
        out["config"]["workload"] += (f"; localBA (set-up + solve + update) per keyframe job on {len(ba.flat)} DISTINCT device-resident "
                                      f"maps around {a.ba_kfs} KFs / {a.ba_lms} landmarks (+-{int(100 * a.ba_spread)} %)")

    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, wl, ba)

    if rank == 0 and a.full and not a.no_roofline:
        # second, instrumented pass over the same steps: every launch bracketed by hipEvents on the ctx stream
        ctx.kernel_timing(True)
        ctx.kernel_times()
        t1 = time.perf_counter()
        n_instr = max(2 * a.kf_every, min(nbatches, a.instr_batches))
        for _ in range(n_instr):
            wl.step(a.kf_every)
        ctx.synchronize()
        el_instr = time.perf_counter() - t1
        times = ctx.kernel_times()
        ctx.kernel_timing(False)
        # algorithmic bytes per launch: KLT from the executed work words of a representative pass over the cycle
        n = wl.n
        per_pos = []
        lk_passes = lk_iters = 0.0
        for _ in range(wl.L):
            cpos = wl.step_no % wl.L
            wl.step(10 ** 9, want_work=True)      # no KF => work words belong to the temporal launch
            ctx.synchronize()
            w = wl.work.get()
            hp = wl.has_host[cpos]
            # first launch: keypoints with a prior (2 levels) + keypoints without (full pyramid); second: re-tracked failures
            wa = np.concatenate([w[:n], w[n:][~hp]])
            wb = w[n:][hp]
            per_pos.append((lk_bytes(wa), lk_bytes(wb), lk_ops(wa), lk_ops(wb)))
            wall = np.concatenate([wa, wb]).astype(np.uint32)
            lk_passes += float((wall >> 16).sum()); lk_iters += float((wall & 0xffff).sum())
        b1 = float(np.mean([p[0] for p in per_pos]))
        b2 = float(np.mean([p[1] for p in per_pos]))
        ops = {"klt_stage1_kernel": float(np.mean([p[2] for p in per_pos])),
               "klt_stage2_kernel": float(np.mean([p[3] for p in per_pos]))}
        lvl_bytes = pyr_level_bytes(W, H, NLVL + 1)
        alg = {
            "klt_stage1_kernel": b1, "klt_stage2_kernel": b2,
            "level_kernel": a.seqs * float(np.mean(lvl_bytes[1:] or lvl_bytes)),   # the separate pyrDown launches: levels 1 -> 2, 2 -> 3
            # level 0 is fused with the first pyrDown: image read + level 0 written + level 1 written
            "level0_kernel": a.seqs * (2.0 * W * H + float(((W + 1) // 2) * ((H + 1) // 2))),
            "clahe_lut_kernel": a.seqs * 1.0 * W * H,
            "detect_cell_kernels": a.seqs * 2.0 * W * H * 0.15 / 4.0,   # image + mask of the ~15 % free cells, 4 colour launches
        }
        rl = {}
        for k, (ms, cnt) in times.items():
            avg_s = ms * 1e-3 / max(cnt, 1)
            gbs = alg.get(k, 0.0) / avg_s / 1e9 if avg_s > 0 else 0.0
            rl[k] = {"avg_us": 1e6 * avg_s, "launches": cnt, "total_ms": ms, "alg_bytes_per_launch": alg.get(k),
                     "achieved_GBs": gbs}
            if k in ops and avg_s > 0:
                # LK is L2-resident and bound by integer VALU + gather latency, so its window-op rate
                # against the vector peak is reported beside the (small by construction) HBM fraction
                rl[k]["alg_ops_per_launch"] = ops[k]
                rl[k]["achieved_Tops"] = ops[k] / avg_s / 1e12
                rl[k]["valu_frac"] = rl[k]["achieved_Tops"] / VALU_PEAK_TOPS
        # The dominant kernel of the path is the combined tracking launch (rocprofv3 trace of this command:
        # profiles/r02_noba_kernel_stats.csv, 33 % of the GPU time against 29 % for the level-0 kernel).  The hipEvent
        # totals of two overlapping streams include each other's queueing and can rank the two either way from run to
        # run, so the choice is made by name; every kernel's own figures are in `kernels`.
        dom = "klt_stage1_kernel" if "klt_stage1_kernel" in times else max(times, key=lambda k: times[k][0])
        # HBM traffic cannot be counted from inside the process: the figure comes from the committed rocprofv3 PMC passes of
        # this same command (profiles/pmc_summary.json, FETCH_SIZE / WRITE_SIZE in separate runs) and is labelled as such
        traffic, traffic_src = None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_summary.json")
        if os.path.exists(pmc):
            try:
                traffic = json.load(open(pmc)).get(dom, {}).get("hbm_bytes_per_launch")
                traffic_src = "profiles/pmc_summary.json (rocprofv3 --pmc passes of this command, not measured in this run)"
            except Exception:
                traffic = None
        out["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": rl[dom]["achieved_GBs"], "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": rl[dom]["achieved_GBs"] / HBM_PEAK_GBS, "traffic": traffic,
                           "traffic_source": traffic_src,
                           "limiter": "integer VALU issue, not HBM (profiles/*_klt_counters.md); the HBM fraction is reported "
                                      "because the contract asks for it, `valu` is the fraction that bounds the kernel",
                           "avg_launch_us": rl[dom]["avg_us"], "alg_bytes_per_launch": rl[dom]["alg_bytes_per_launch"]}
        # the hipEvent pass above runs after the BA worker has stopped; inside the timed region the same kernel shares the
        # device with the worker's batches: its average there comes from the committed rocprofv3 kernel trace of this command
        try:
            import csv as _csv
            for fn in sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_kernel_stats.csv") and "noba" not in f):
                for row in _csv.DictReader(open(os.path.join(ROOT, "profiles", fn))):
                    if row.get("Name") == dom:
                        avg_ns = float(row["AverageNs"])
                        out["roofline"]["in_region"] = {"avg_launch_us": avg_ns / 1e3, "frac": rl[dom]["alg_bytes_per_launch"] / (avg_ns * 1e-9) / 1e9 / HBM_PEAK_GBS,
                                                        "source": f"profiles/{fn} (rocprofv3 --kernel-trace --stats of this command, BA worker concurrent; "
                                                                  "not measured in this run)"}
        except Exception:
            pass
        if "valu_frac" in rl[dom]:
            out["roofline"]["valu"] = {"achieved": rl[dom]["achieved_Tops"], "peak": VALU_PEAK_TOPS, "unit": "Tiop/s",
                                       "frac": rl[dom]["valu_frac"]}
        out["kernels"] = rl
        # executed LK work of the temporal tracking (work words of the kernels): how hard the stream is
        out["config"]["lk_level_passes_per_keypoint"] = lk_passes / (wl.L * n)
        out["config"]["lk_iterations_per_level_pass"] = lk_iters / max(lk_passes, 1.0)
        out["config"]["frame_gap"], out["config"]["prior_sigma_px"] = a.frame_gap, a.prior_sigma
        out["config"]["stream_priority"] = {"front_end": a.fe_priority, "local_ba": a.ba_priority}
        out["ms_per_frame_batch_instrumented"] = 1e3 * el_instr / n_instr

    if rank == 0 and a.full and not a.no_roofline and not a.no_hard_stream:
        # a HARDER stream beside the headline one (front-end alone, outside the timed region): three times the flow per
        # frame and priors 3 px off, so the LK passes iterate about twice as often -- how the rate degrades with difficulty
        hw = Workload(ctx, fe, synth, a.seqs, a.kps, 4, seed=synth.SEED_IMG + 101 * rank + 7, gap=3 * a.frame_gap,
                      prior_sigma=3.0 * a.prior_sigma)
        for _ in range(2 * hw.L):
            hw.step(a.kf_every)
        ctx.synchronize()
        nb_h = max(4 * a.kf_every, min(120, nbatches))
        t1 = time.perf_counter()
        for _ in range(nb_h):
            hw.step(a.kf_every)
        ctx.synchronize()
        el_h = time.perf_counter() - t1
        hp_, hi_ = 0.0, 0.0
        for _ in range(hw.L):
            hw.step(10 ** 9, want_work=True)
            ctx.synchronize()
            wv = hw.work.get()
            hp_ += float((wv >> 16).sum()); hi_ += float((wv & 0xffff).sum())
        tracked = float(hw.out_st.get().mean())
        out["hard_stream"] = {"frames_per_sec_front_end_alone": nb_h * a.seqs / el_h, "frame_gap": 3 * a.frame_gap,
                              "prior_sigma_px": 3.0 * a.prior_sigma, "lk_level_passes_per_keypoint": hp_ / (hw.L * hw.n),
                              "lk_iterations_per_level_pass": hi_ / max(hp_, 1.0), "tracked_fraction": tracked,
                              "frame_batches": nb_h,
                              "note": "same pipeline on a stream with 3x the flow and 3x the prior error; no BA worker beside it"}
        del hw

    if rank == 0 and a.full and not a.no_roofline and not a.no_euroc_like:
        # The size the reference actually runs (configs 2 / 3: <= 308 keypoints per frame = nmaxdist 35 on 752 x 480,
        # src/slam_params.cpp:107-110; windows of 10-30 keyframes / 1-3 k landmarks, ONE sequence): the same pipeline with
        # per-frame ceresPnP on the tracking stream and the whole local BA (set-up + solve + update) per keyframe beside it,
        # for 1 and for 8 sequences.  Outside the timed region.
        from ov2slam_amd import synth_ba as _sb
        out["euroc_like"] = {"keypoints_per_frame": 308, "detector_cell": 35, "kf_every": a.kf_every,
                             "ba_window_nominal": {"keyframes": 20, "landmarks": 2000},
                             "note": "device-resident inputs; per-frame ceresPnP on; local BA = set-up + solve + update on the "
                                     "sequence's own device map, concurrent; one frame-batch = one new stereo frame of every sequence"}
        for nseq in (1, 8):
            try:
                ew = Workload(ctx, fe, synth, nseq, 308, 8, seed=synth.SEED_IMG + 977 * nseq, gap=a.frame_gap, prior_sigma=a.prior_sigma,
                              det_cell=35)
                ew.enable_pnp(seed=4242 + nseq)
                esp = _sb.sequence_window_specs(nseq, seed=515 + nseq, n_kf=20, n_lm=2000, spread=0.3)
                eba = BaPipeline(fe, local, _sb.make_windows_parallel(esp, 1 if nseq == 1 else 8), esp, workers=1, max_batch=64,
                                 high_priority=a.ba_priority == "high")
                for _ in range(4 * ew.L):
                    if ew.step(a.kf_every):
                        eba.submit_all()
                ctx.synchronize()
                eba.set_counting(True)
                nfb = 1200
                t1 = time.perf_counter()
                for _ in range(nfb):
                    if ew.step(a.kf_every):
                        eba.submit_all()
                ctx.synchronize()
                el_py = time.perf_counter() - t1
                # the same frames enqueued by the native driver (libov2host.so: ov2h_feloop_run issues the identical sequence
                # of ABI calls from C++; a 308-keypoint frame is ~12 launches, the interpreter's share of each call is what
                # bounds the loop above).  This is the leg's figure; the interpreter-driven one is kept beside it.
                from ov2slam_amd import host_map as _hm
                ew.prev.release(); ew.prev = None
                floop = _hm.FrameLoop(ctx, ew, WIN, NLVL, fe.clahe_tiles(W, H), eba.ws)
                floop.run(4 * ew.L, a.kf_every)
                ctx.synchronize()
                base_t = eba.refresh()
                t1 = time.perf_counter()
                floop.run(nfb, a.kf_every)
                ctx.synchronize()
                el_e = time.perf_counter() - t1
                eba.set_counting(False)
                et = eba.refresh()
                et = {k: (et[k] - base_t[k] if isinstance(et[k], (int, float)) else et[k]) for k in et}
                eba.stop()
                floop.close()
                # the front-end chain alone, one frame at a time with a synchronisation after each: the latency a single
                # camera sees (pyramid + two-stage KLT + ceresPnP)
                ew.detect = False
                lat = []
                for _ in range(60):
                    ctx.synchronize()
                    t2 = time.perf_counter()
                    ew.step(10 ** 9)
                    ctx.synchronize()
                    lat.append(time.perf_counter() - t2)
                out["euroc_like"][f"{nseq}_seq"] = {
                    "frames_per_sec": nfb * nseq / el_e, "ms_per_frame_batch": 1e3 * el_e / nfb,
                    "frames_per_sec_per_sequence": nfb / el_e,
                    "host_driver": "native (ov2h_feloop_run, C++ over the C ABI)",
                    "frames_per_sec_python_driver": nfb * nseq / el_py,
                    "frame_latency_ms_median": 1e3 * float(np.median(lat)),
                    "tracked_fraction": float(ew.out_st.get().mean()),
                    "local_ba": {"solves_per_sec": et["solves"] / el_e, "lm_iterations_per_sec": et["iters"] / el_e,
                                 "ms_per_batch": 1e3 * et["busy_s"] / max(et["batches"], 1), "windows_per_batch": et["solves"] / max(et["batches"], 1),
                                 "replaced_fraction": et["dropped"] / max(et["submitted"], 1),
                                 "residual_blocks_mean": float(np.mean([f["residual_blocks"] for f in eba.flat])),
                                 "poses_mean": float(np.mean([f["poses"] for f in eba.flat]))}}
                if nseq == 1 and not a.no_cpu_baseline and world == 1:
                    from oracle import oracle_py as O
                    O.use_native(True)
                    legs = {}
                    for t in (1, 16):
                        fps, nfr, sec = cpu_baseline(ew, a.kf_every, min(a.cpu_seconds, 5.0), threads=t)
                        legs[str(t)] = {"value": fps, "unit": "frames/s", "cores": t, "sample": f"{nfr} frames ({sec:.1f} s)"}
                    out["euroc_like"]["cpu_baseline"] = {"kind": "port", "by_threads": legs,
                                                         "note": "oracle/ C port of the OpenCV path on the same 308-keypoint stream (CLAHE + pyramid + "
                                                                 "two-stage KLT per frame, right pyramid + stereo KLT per keyframe; no PnP / BA)"}
                    try:   # ... and the local BA of the same EuRoC-sized window on one host thread
                        pe = eba.flat_problems(1)
                        t3 = time.perf_counter()
                        nso, itso = 0, 0
                        while time.perf_counter() - t3 < 3.0:
                            Rc = O.ba_solve(pe[0].copy())
                            itso += sum(Rc.summary()["iterations"]); nso += 1
                        dtb = time.perf_counter() - t3
                        out["euroc_like"]["cpu_baseline"]["local_ba"] = {
                            "solves_per_sec": nso / dtb, "lm_iterations_per_sec": itso / dtb, "cores": 1, "kind": "port",
                            "sample": f"{nso} solves of the 1-sequence leg's window ({pe[0].n_res} residual blocks; solve stage only) in {dtb:.1f} s"}
                    except Exception as e2:
                        out["euroc_like"]["cpu_baseline"]["local_ba"] = {"error": repr(e2)}
                del ew, eba
            except Exception as e:   # a side report: never lose the bench line to it
                out["euroc_like"][f"{nseq}_seq"] = {"error": repr(e)}

    do_cpu = a.full and rank == 0 and world == 1 and not a.no_cpu_baseline   # the CPU leg is reported at N = 1 only
    if do_cpu:
        from oracle import oracle_py as O
        native = O.use_native(True)        # same sources at -O3 -march=native for this host
        try:
            share = len(os.sched_getaffinity(0))
        except Exception:
            share = os.cpu_count() or 1
        # one thread per host core this process may run on (OpenCV's parallel_for_ default); the 16-thread and the
        # 1-thread figures beside it
        nthr = a.cpu_threads if a.cpu_threads > 0 else max(1, share)
        legs = {}
        for t in sorted({1, min(16, nthr), min(64, nthr), nthr}):
            fps, nfr, sec = cpu_baseline(wl, a.kf_every, a.cpu_seconds, threads=t)
            legs[t] = {"value": fps, "unit": "frames/s", "cores": t, "sample": f"{nfr} frames ({sec:.1f} s), same build, {t} thread(s)"}
        build = "-O3 -march=native" if native else "-O2 (native build failed)"
        quota = None   # the container's CPU share (cgroup v2 cpu.max), when it is less than the cores the affinity mask shows
        try:
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
        except Exception:
            pass
        # The line's value is the FASTEST of the legs (the strongest baseline this host gives); the one-thread-per-visible-core
        # leg SURVEY 8d names is kept beside it as `all_cores` (on a box whose CPU share is smaller than the cores it shows,
        # that leg is oversubscribed and slower than 16 threads)
        best_t = max(legs, key=lambda t: legs[t]["value"])
        out["cpu_baseline"] = {"value": legs[best_t]["value"], "unit": "frames/s", "cores": best_t, "kind": "port",
                               "sample": legs[best_t]["sample"] + f" of one sequence of the same workload, oracle/ C port of "
                                         f"the OpenCV path built {build}, threads split the points of every LK call and "
                                         "the rows / tiles of CLAHE, pyrDown and Scharr (cv::parallel_for_); fastest of the "
                                         f"legs in by_threads; host has {os.cpu_count()} logical cores, {share} in the affinity "
                                         f"mask, cgroup CPU quota {quota if quota is not None else 'none'}",
                               "single_thread": legs[1],
                               "all_cores": legs[nthr],
                               "by_threads": {str(t): v for t, v in legs.items()},
                               "best": legs[best_t]}
    if do_cpu and ba and legacy_ba:
        Pc = ba.P0.copy()
        t1 = time.perf_counter()
        Rc = O.ba_solve(Pc)
        dt = time.perf_counter() - t1
        out["local_ba"]["cpu_baseline"] = {"value": sum(Rc.summary()["iterations"]) / dt, "unit": "iters/s", "cores": 1,
                                           "kind": "port", "sample": f"one solve of the same window ({dt:.2f} s), "
                                           "oracle/ C restatement of the Ceres LM + Schur path, 1 thread "
                                           "(the reference runs localBA with num_threads = 1, src/optimizer.cpp:460)"}
    elif do_cpu and ba:
        # the CPU port on the SAME distinct windows: the flat problems the device set-up makes of the first maps, solved one
        # after the other by the oracle (1 thread: the reference runs localBA with num_threads = 1) until the budget is spent
        try:
            probs = ba.flat_problems(min(len(ba.flat), 48))
            t1 = time.perf_counter()
            its, nsolved = 0, 0
            for Pc in probs:
                Rc = O.ba_solve(Pc)
                its += sum(Rc.summary()["iterations"]); nsolved += 1
                if time.perf_counter() - t1 > a.cpu_seconds:
                    break
            dt = time.perf_counter() - t1
            out["local_ba"]["cpu_baseline"] = {"value": its / dt, "unit": "iters/s", "solves_per_sec": nsolved / dt, "cores": 1,
                                               "kind": "port",
                                               "sample": f"the solve stage of the first {nsolved} of the same distinct windows "
                                               f"({dt:.1f} s; the flat problems the device set-up produced), oracle/ C restatement "
                                               "of the Ceres LM + Schur path, 1 thread (the reference runs localBA with "
                                               "num_threads = 1, src/optimizer.cpp:460); set-up and update of the host mirror are in `setup`"}
        except Exception as e:
            out["local_ba"]["cpu_baseline"] = {"error": repr(e)}
    if do_cpu and ba:
        # set-up stage of Optimizer::localBA on a map holding one of the windows: the reference-style hash-map walk (C++
        # host mirror, this host's core) beside the one-map form of the device scans (whole call: scans, 2 syncs, D2H of
        # the flat problem, host id maps).  Outside the timed region; reported, not part of `value`.
        try:
            import ctypes as C
            from ov2slam_amd import host_map
            hm = host_map.HostMap(ba.P0 if legacy_ba else windows[0])
            hm.attach_device(ctx)
            HL = host_map.lib()
            na, nb, nc = C.c_int(), C.c_int(), C.c_int()

            def t_setup(fn, reps=10):
                fn(hm.h, hm.newkf, C.byref(na), C.byref(nb), C.byref(nc))
                t = time.perf_counter()
                for _ in range(reps):
                    fn(hm.h, hm.newkf, C.byref(na), C.byref(nb), C.byref(nc))
                return 1e3 * (time.perf_counter() - t) / reps
            out["local_ba"]["setup"] = {"hash_map_walk_ms": t_setup(HL.ov2h_local_ba_setup),
                                        "device_map_scans_one_map_ms": t_setup(HL.ov2h_local_ba_setup_dev),
                                        "problem": {"poses": na.value, "landmarks": nb.value, "residual_blocks": nc.value},
                                        "note": "src/optimizer.cpp:43-430; walk = C++ mirror of the reference's maps on 1 host core; "
                                                "the batched form inside the timed region is local_ba.ms_per_batch.setup_per_window"}
            del hm
        except Exception as e:   # the set-up comparison is a side report: never lose the bench line to it
            out["local_ba"]["setup"] = {"error": repr(e)}
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
