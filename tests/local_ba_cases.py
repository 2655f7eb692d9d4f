"""Window-solve fixtures (LocalBundleAdjustmentNavState and LocalBundleAdjustment) that leave the straight road of "every trial accepted,
5 + 10 iterations": named recipes — a synth generator call plus deterministic post-processing, no stored arrays — each tagged with the
path through the Levenberg rule (csrc/lm_core.h) it is there for. tests/test_local_ba_cases.py proves on the CPU oracle alone that every
fixture does what its tag says and that none of its decisions sits on a jump; tests/test_gpu_local_ba_cases.py runs them through the four
drivers of csrc/local_ba.hip.

A recipe: kind ("nav" | "se3"), gen (keyword arguments of make_local_ba_problem / make_local_ba_se3_problem), and optionally
  noise = (rng_seed, sigma): points += numpy.random.default_rng(rng_seed).normal(0, sigma, points.shape)
  restart = True: the window is first solved by the oracle, and the fixture starts from that solution (key frames and points)
  noise_tail = True: the second optimize() runs on into rounding noise (chi2 1e-25), where accept or reject hangs on the last bits of two
    sums. Only the trial rows before the first one whose chi_before is below NOISE_CHI2 are decidable (decidable_rows); its_second and the
    numbers of trials and of rejected trials are not compared, and chi2_final is only required to be below NOISE_CHI2 too."""
import numpy as np

NOISE_CHI2 = 1e-12
TAGS = ("stall_stop", "stall_reset", "restart", "failed_solve_qmax", "all_gated", "mid_reject_retry", "late_reject", "plain")


def _nav(seed, W, n_points, **kw):
    return dict(seed=seed, W=W, n_points=n_points, n_fixed_extra=2, **kw)


def _se3(seed, W, n_points, stereo_frac, **kw):
    return dict(seed=seed, W=W, n_fixed=2, n_points=n_points, stereo_frac=stereo_frac, **kw)


_QUIET = dict(pix_sigma=0.05, outlier_frac=0.0)

CASES = [
    # early stop by the stall rule: nBad reaches 3 in the second optimize() (5 + 3 iterations)
    dict(name="nav_stall_32", tag="stall_stop", kind="nav", gen=_nav(32, 5, 200, **_QUIET)),
    dict(name="se3_stall_44", tag="stall_stop", kind="se3", gen=_se3(44, 2, 60, 0.0, **_QUIET)),
    # stalled iterations that do not follow each other: in the second optimize() two iterations stall, two gain again (nBad back to 0), then
    # three stall and end it after 9 of 10 (a restarted noisy window)
    dict(name="nav_stall_reset_223", tag="stall_reset", kind="nav", gen=_nav(223, 3, 90, pix_sigma=1.0, outlier_frac=0.05), restart=True),
    # started from its own solution: the stall rule ends the first optimize() too (3 + 3 iterations), or the second alone
    # (se3_restart_44, a noisy window: 5 + 8)
    dict(name="nav_restart_32", tag="restart", kind="nav", gen=_nav(32, 5, 200, **_QUIET), restart=True),
    dict(name="se3_restart_40", tag="restart", kind="se3", gen=_se3(40, 5, 200, 0.0, **_QUIET), restart=True),
    dict(name="se3_restart_44", tag="restart", kind="se3", gen=_se3(44, 3, 90, 0.0), restart=True),
    # the gate after the first optimize() removes every edge: the reduced system is zero, the factorisation fails, ten trials with
    # rho = -inf, Terminate on qmax == 10 (5 + 1 iterations, chi2_final 0, all edges erased)
    dict(name="se3_failed_42", tag="failed_solve_qmax", kind="se3", gen=_se3(42, 6, 300, 0.0), noise=(42, 7.0)),
    dict(name="se3_failed_45", tag="failed_solve_qmax", kind="se3", gen=_se3(45, 3, 100, 0.3), noise=(45, 6.0)),
    # the gate after the first optimize() removes every edge of a NavState window: the IMU and bias factors remain, the solves succeed, no
    # point has an active edge, and chi2 falls 8e3 -> 1e-25. Three trials of the second optimize() are decidable, the rest is noise (there the
    # oracle takes 17 more trials and rejects 10 of them)
    dict(name="nav_all_gated_34", tag="all_gated", kind="nav", gen=_nav(34, 3, 90), noise=(4, 4.0), noise_tail=True),
    # rejected trials in the middle of a solve, all of them in the first optimize(); up to 3 (NavState) and 5 (SE3) trials in one iteration
    dict(name="nav_mid_122", tag="mid_reject_retry", kind="nav", gen=_nav(122, 3, 90), noise=(122, 2.0)),
    dict(name="nav_mid_131", tag="mid_reject_retry", kind="nav", gen=_nav(131, 1, 40), noise=(131, 0.5)),
    dict(name="nav_mid_126", tag="mid_reject_retry", kind="nav", gen=_nav(126, 3, 90), noise=(126, 1.0)),
    dict(name="se3_mid_153", tag="mid_reject_retry", kind="se3", gen=_se3(153, 3, 90, 0.0), noise=(153, 2.0)),
    dict(name="se3_mid_126", tag="mid_reject_retry", kind="se3", gen=_se3(126, 3, 90, 0.0), noise=(126, 2.0)),
    # two rejected trials in the last iteration of the second optimize() (rho -3.58 and -614), then an accepted one
    dict(name="nav_late_4", tag="late_reject", kind="nav", gen=_nav(4, 1, 60)),
    # the straight road: 5 + 10 iterations, 15 trials, none rejected
    dict(name="nav_plain_13", tag="plain", kind="nav", gen=_nav(13, 3, 90)),
    dict(name="se3_plain_2", tag="plain", kind="se3", gen=_se3(2, 4, 120, 0.0)),
]

BY_NAME = {c["name"]: c for c in CASES}


def preints(oracle, p):
    out = []
    for i, (imu, t0, t1) in enumerate(p["imu"]):
        j = i - 1 if i > 0 else p["prev_kf"]
        out.append(oracle.preintegrate(imu, p["kfs"][j][10:13], p["kfs"][j][13:16], t0, t1))
    return np.stack(out)


def solve_oracle(oracle, kind, args):
    return oracle.local_ba(**args) if kind == "nav" else oracle.local_ba_se3(**args)


def build(case, oracle):
    """The solver arguments of a fixture, as keyword arguments shared by the oracle's and the device's entry points."""
    from viorb_amd.synth import make_local_ba_problem, make_local_ba_se3_problem
    if case["kind"] == "nav":
        p = make_local_ba_problem(**case["gen"])
        args = dict(kfs=p["kfs"].copy(), n_local=p["n_local"], prev_kf=p["prev_kf"], preint=preints(oracle, p), points=p["points"].copy(),
                    edge_idx=p["edge_idx"], edge_obs=p["edge_obs"], gw=p["gw"], cam=p["cam"])
    else:
        p = make_local_ba_se3_problem(**case["gen"])
        args = dict(kfs=p["kfs"].copy(), n_local=p["n_local"], points=p["points"].copy(), edge_idx=p["edge_idx"], edge_obs=p["edge_obs"], intr5=p["intr5"])
    if case.get("noise"):
        rng_seed, sigma = case["noise"]
        args["points"] = args["points"] + np.random.default_rng(rng_seed).normal(0, sigma, args["points"].shape)
    if case.get("restart"):
        r = solve_oracle(oracle, case["kind"], args)
        args["kfs"][:args["n_local"]] = r["kfs"]
        args["points"] = r["points"].copy()
    return args


def accepted(trials):
    """Per trial row of oracle.binding (BA_TRIAL_COLUMNS): rho > 0 and a finite tempChi."""
    return (trials[:, 4] > 0) & np.isfinite(trials[:, 5])


def decidable_rows(case, trials):
    """How many leading trial rows of a fixture are held to the oracle: all, or for a noise_tail fixture those before chi2 reaches noise
    (chi_before is the same for every trial of an iteration, so the cut falls between two iterations)."""
    if not case.get("noise_tail"):
        return len(trials)
    low = np.flatnonzero(trials[:, 7] < NOISE_CHI2)
    return int(low[0]) if len(low) else len(trials)


def trials_per_iteration(trials):
    """{(phase, iteration): number of trials}"""
    out = {}
    for r in trials:
        k = (int(r[0]), int(r[1]))
        out[k] = out.get(k, 0) + 1
    return out
