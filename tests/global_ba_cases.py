"""The problems the GPU tests of the global bundle adjustment solve (tests/test_gpu_global_ba.py) and the CPU margin test vets
(tests/test_global_ba_ref.py): N key frames with about 40 points each, robust 0 / 1, revisit_frac 0 / 0.2, 10 iterations."""
import numpy as np

ITERATIONS = 10
# (seed, N, robust, revisit_frac)
CASES = [(100 + 10 * i + 2 * r + (1 if f else 0), N, r, f) for i, N in enumerate((3, 21, 60, 128, 256)) for r in (0, 1) for f in (0.0, 0.2)]
# the problems of the other GPU tests that are compared with the checker (or with a solo run), all generated with revisit_frac 0
THREAD_SEEDS = [(301, 12), (302, 16), (303, 9), (304, 20)]          # (seed, N): four concurrent callers, robust, 10 iterations
STOP_SEED, DEGENERATE_SEED, FIXED_SEED = (311, 21), (312, 21), (304, 20)
FIXED_ITERATIONS = 5


def degenerate_points_variant(p):
    """point 5 keeps a single observation, point 9 loses all of them, and a trailing point nobody observes is added"""
    ei, eo = p["edge_idx"], p["edge_obs"]
    keep = np.ones(len(ei), bool)
    keep[np.flatnonzero(ei[:, 0] == 5)[1:]] = False
    keep[ei[:, 0] == 9] = False
    return dict(p, edge_idx=ei[keep], edge_obs=eo[keep], points=np.vstack([p["points"], [[0.5, -0.25, 4.0]]]))


def fixed_inside_variant(p):
    """two more fixed key frames: 1 (so that the IMU factor 0 -> 1 joins two fixed ones) and 11 in the middle of the graph"""
    fixed = p["fixed"].copy(); fixed[1] = 1; fixed[11] = 1
    return dict(p, fixed=fixed)


def checked_variants(problem):
    """every (name, problem, robust, iterations) a GPU test holds the device to the checker on besides CASES; problem(seed, N) builds one"""
    out = [("threads-%d" % s, problem(s, N), 1, ITERATIONS) for s, N in THREAD_SEEDS]
    out += [("degenerate-%d" % r, degenerate_points_variant(problem(*DEGENERATE_SEED)), r, ITERATIONS) for r in (0, 1)]
    out.append(("fixed-inside", fixed_inside_variant(problem(*FIXED_SEED)), 1, FIXED_ITERATIONS))
    return out


def oracle_preint(oracle):
    """preint_fn for synth.make_global_ba_problem on a machine without a device: the oracle's pre-integrator, interval by interval."""
    def fn(s, bg, ba):
        n = len(s["kf_time"]); out = np.zeros((n, 142))
        for i in range(1, n):
            out[i] = oracle.preintegrate(s["imu"][s["imu_start"][i]:s["imu_start"][i + 1]], bg, ba, s["kf_time"][i - 1], s["kf_time"][i])
        return out
    return fn


def args(p):
    return (p["kfs"], p["prev"], p["fixed"], p["preint"], p["points"], p["edge_idx"], p["edge_obs"], p["gw"], p["cam"])
