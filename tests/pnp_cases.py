"""Pose-refinement frames whose initial pose is far off (0.8 rad, 2 m): the LM loop of MultiViewGeometry::ceresPnP
rejects steps and cuts its radius before it converges, or never finds an acceptable step.  Shared by
tests/test_pnp_cases_cpu.py (the rejection shown on the oracle, tameness), tests/test_pnp_gpu.py (parity) and
scripts/oracle_cov.py."""
from ov2slam_amd import synth_ba

SEEDS = (0, 1, 2)
MAX_ITERS = 10


def far_off_frame(seed):
    return synth_ba.make_pnp(200, seed, outlier_frac=0.1, rot_pert=0.8, trans_pert=2.0)


def solve_oracle(oracle, p, Twc0=None, **kw):
    """(success, Twc, outlier mask, (robust iterations, L2 iterations)) of the oracle"""
    kw.setdefault("max_iters", MAX_ITERS)
    return oracle.pnp_solve(p["unpx"], p["wpts"], p["K"], p["Twc0"] if Twc0 is None else Twc0, p["scales"], **kw)


def cases():
    return [far_off_frame(s) for s in SEEDS]


def run(case, oracle):
    """what scripts/oracle_cov.py calls for every case"""
    return solve_oracle(oracle, case)
