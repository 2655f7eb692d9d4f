"""The window-solve fixtures of tests/local_ba_cases.py, proved on the CPU oracle alone (oracle/local_ba.cpp, oracle/local_ba_se3.cpp):
every fixture takes the path through the Levenberg rule its tag names, and none of its decisions sits on a jump, so that the device
(tests/test_gpu_local_ba_cases.py) can be held to the oracle's accept / reject sequence trial by trial.

Decidable means: solved 8 more times with its points scaled by 1 + 1e-9 N(0, 1) — the size of the run-to-run difference the batch
tests grant the device — a fixture gives the same trial rows in phase, iteration, qmax and the solved / accepted flags, and the same
erase flags; and inside the rows
  * no finite rho is closer to 0 than M,
  * no stall test "(iniChi - currentChi) * 1e3 < iniChi" is closer to equality than M, relative: |(iniChi - currentChi) * 1e3 / iniChi - 1| >= M.
M is 100 x the largest change the perturbation makes, over all fixtures, perturbed solves and trials, in rho (relative, |d rho| / |rho|)
and in the stall quantity (iniChi - currentChi) * 1e3 / iniChi (in units of its threshold, 1).
Measured over the 17 fixtures x 8 perturbed solves: rho moves by at most 1.4e-5 (nav_mid_126), the stall quantity by at most 2.02e-4
(se3_failed_45, the one fixture with stereo edges); M = 100 x 2.02e-4, rounded up: 2.1e-2. (Each fixture's perturbations are drawn from a
generator seeded by its name, so the figures do not move when the list changes.) The smallest margins kept are |rho| >= 0.0648
(nav_restart_32) and |stall - 1| >= 0.153 (nav_plain_13).

Thrown away, and why. Sensitive: vision-only windows with stereo edges (the float reciprocal depth of EdgeStereoSE3ProjectXYZ) move far
more under the perturbation than the others and would have raised M above every margin: stall_stop SE3 (48, 3, 90, stereo 0.5) moved
rho by 7.1e-2, restart SE3 (43, 5, 200, stereo 1.0) by 1e-3 with a stall margin of 0.074, mid_reject_retry SE3 (136, 1, 40, stereo 0.5)
moved the stall quantity by 1.4e-3 and (128, 1, 40, stereo 1.0) by 2.4e-3. Their places went to monocular windows. Too close: NavState
(31, 3, 90) as stall_stop and restart has |rho| = 0.0148 and 0.0144, below M = 2.1e-2; (32, 5, 200) stands for both.

The tag "all_gated" (every edge gated after the first optimize(), the solves of the second succeed) is held to the oracle in part. It can
only be a NavState window (a vision-only window without edges has a zero system: failed_solve_qmax). Its second optimize() has nothing
but the IMU and bias factors left, which the key frames can meet exactly, so chi2 falls to rounding noise (1e-25) within the ten
iterations, and the last trials have |rho| below 1e-20: accept or reject is then decided by the last bits of two sums. NavState
(33, 6, 300), (34, 3, 90) and (35, 2, 60) with points moved by sigma 3 and 4 under numpy.random.default_rng(0 .. 49) gave 96 windows that
erase every edge; every one ends that way, and most reject 4 to 12 trials there (the mid-solve candidates NavState (120, 3, 90),
(125, 1, 40), (139, 3, 90), (150, 3, 90), (151, 3, 90) with sigma 1 to 2 too: thrown away). So the fixture kept, nav_all_gated_34 = (34, 3, 90)
with default_rng(4) and sigma 4, is marked noise_tail: its rows count up to the first trial whose chi_before is below 1e-12 (8 of 25: the
five of the first optimize() and three of the second, |rho| >= 0.922), on which everything above is proved; its_second and the numbers
of trials and of rejected trials are not compared, here or on the device. Of the draws of (34, 3, 90), default_rng(2) / sigma 3, 9 / 3 and
16 / 3 have a smaller |rho| in their prefix (0.19, 0.12, 0.09) and 2 / 4, 10 / 3, 12 / 4 one below M."""
import zlib

import numpy as np
import pytest

import local_ba_cases as LC

N_PERTURBED = 8
M = 2.1e-2

# what the table of fixtures must hold: tag -> {kind: at least}
REQUIRED = {"stall_stop": {"nav": 1, "se3": 1}, "stall_reset": {"nav": 1}, "restart": {"nav": 1, "se3": 1}, "failed_solve_qmax": {"se3": 1},
            "all_gated": {"nav": 1},             "mid_reject_retry": {"nav": 2, "se3": 2}, "late_reject": {"nav": 1}, "plain": {"nav": 1, "se3": 1}}


def iterations_of(trials):
    """Per iteration, in order: dict(phase, it, n (trials), ini (iniChi), cur (currentChi at its end), rho, terminated (qmax == 10 or rho == 0),
    stall = (iniChi - currentChi) * 1e3 / iniChi (None when iniChi is 0))."""
    acc = LC.accepted(trials)
    out = []
    for i, r in enumerate(trials):
        if not out or (out[-1]["phase"], out[-1]["it"]) != (int(r[0]), int(r[1])):
            out.append(dict(phase=int(r[0]), it=int(r[1]), n=0, ini=r[7], cur=r[7]))
        e = out[-1]
        e["n"] += 1; e["rho"] = r[4]
        if acc[i]:
            e["cur"] = r[5]
    for e in out:
        e["terminated"] = e["n"] == 10 or e["rho"] == 0
        e["stall"] = (e["ini"] - e["cur"]) * 1e3 / e["ini"] if e["ini"] != 0 else None
    return out


@pytest.fixture(scope="module")
def solved(oracle):
    """name -> (case, base result, the perturbed results); every oracle solve of this module happens here, once."""
    out = {}
    for case in LC.CASES:
        args = LC.build(case, oracle)
        base = LC.solve_oracle(oracle, case["kind"], args)
        rng = np.random.default_rng(zlib.crc32(case["name"].encode()))     # a fixture's draws do not depend on its place in the list
        pert = []
        for _ in range(N_PERTURBED):
            a = dict(args); a["points"] = args["points"] * (1 + 1e-9 * rng.normal(0, 1, args["points"].shape))
            pert.append(LC.solve_oracle(oracle, case["kind"], a))
        out[case["name"]] = (case, base, pert)
    return out


def _flags(t):
    return np.column_stack([t[:, :4], LC.accepted(t)]).astype(np.int64)


def test_table_is_filled():
    names = [c["name"] for c in LC.CASES]
    assert len(set(names)) == len(names)
    for c in LC.CASES:
        assert c["tag"] in LC.TAGS and c["kind"] in ("nav", "se3")
        assert c["gen"]["W"] <= 6 and c["gen"]["n_points"] <= 300
    for tag, kinds in REQUIRED.items():
        for kind, least in kinds.items():
            assert sum(c["tag"] == tag and c["kind"] == kind for c in LC.CASES) >= least, (tag, kind)
    assert sum(c["tag"] == "plain" for c in LC.CASES) == 2


def test_fixtures_are_decidable(solved):
    """Same rows, same erase flags under the perturbation; rho and the stall test keep the margin M from their thresholds."""
    measured_rho = measured_stall = 0.0
    for name, (case, base, pert) in solved.items():
        k = LC.decidable_rows(case, base["trials"])       # all rows, or those before a noise_tail fixture reaches rounding noise
        t = base["trials"][:k]
        fin = np.isfinite(t[:, 4])
        its = iterations_of(t)
        stalls = np.array([e["stall"] for e in its if not e["terminated"] and e["stall"] is not None])
        margin_rho = np.abs(t[fin, 4]).min() if fin.any() else np.inf
        margin_stall = np.abs(stalls - 1).min() if len(stalls) else np.inf
        d_rho = d_stall = 0.0
        for q in pert:
            tq = q["trials"][:k]
            assert LC.decidable_rows(case, q["trials"]) == k and np.array_equal(_flags(tq), _flags(t)), name
            assert np.array_equal(q["erase"], base["erase"]), name
            assert q["its_first"] == base["its_first"], name
            if not case.get("noise_tail"):
                assert q["trials"].shape == t.shape and q["its_second"] == base["its_second"], name
            assert np.array_equal(np.isfinite(tq[:, 4]), fin), name
            if fin.any():
                d_rho = max(d_rho, (np.abs(tq[fin, 4] - t[fin, 4]) / np.abs(t[fin, 4])).max())
            sq = np.array([e["stall"] for e in iterations_of(tq) if not e["terminated"] and e["stall"] is not None])
            if len(stalls):
                d_stall = max(d_stall, np.abs(sq - stalls).max())
        print("%-16s %-17s its %d+%d trials %2d rejected %2d | margin: |rho| >= %.3g, |stall - 1| >= %.3g | moved by 1e-9: rho %.2g (rel), stall %.2g"
              % (name, case["tag"], base["its_first"], base["its_second"], base["n_trials"], base["n_rejected"], margin_rho, margin_stall, d_rho, d_stall)
              + (" | held to the oracle: the first %d trials" % k if case.get("noise_tail") else ""))
        measured_rho, measured_stall = max(measured_rho, d_rho), max(measured_stall, d_stall)
        assert margin_rho >= M, (name, margin_rho)
        assert margin_stall >= M, (name, margin_stall)
    print("largest change under the perturbation: rho %.3g (relative), stall quantity %.3g; M = %.3g" % (measured_rho, measured_stall, M))
    # M was fixed from these two figures (module docstring); on another host they may differ in the last digits, not by a factor of ten
    # and not by a factor of ten the other way either: M is 100 x the measurement, not a number that once was
    assert 10 * max(measured_rho, measured_stall) <= M <= 1000 * max(measured_rho, measured_stall)


def test_fixtures_take_the_path_of_their_tag(solved):
    seen = {}
    for name, (case, base, _) in solved.items():
        t, tag = base["trials"], case["tag"]
        acc = LC.accepted(t); its = iterations_of(t); rej = ~acc
        budget = {0: 5, 1: 10}
        assert base["n_trials"] == len(t) and base["n_rejected"] == int(rej.sum())
        assert (base["its_first"], base["its_second"]) == (sum(e["phase"] == 0 for e in its), sum(e["phase"] == 1 for e in its))
        if tag in ("stall_stop", "restart"):
            assert not rej.any() and (t[:, 3] == 1).all(), name
            early = [ph for ph in (0, 1) if sum(e["phase"] == ph for e in its) < budget[ph]]
            assert early, name
            for ph in early:                  # the phase ended on nBad == 3: its last three iterations stalled, none of them terminated
                last = [e for e in its if e["phase"] == ph][-3:]
                assert len(last) == 3 and all(not e["terminated"] and e["stall"] < 1 for e in last), name
            if tag == "stall_stop":
                assert base["its_first"] == 5 and base["its_second"] < 10, name
            else:
                assert case.get("restart"), name                  # little left to gain: the stall rule ends a phase (asserted above)
        elif tag == "stall_reset":            # a phase meets three stalled iterations before its end, and goes on because a gaining one lay between them
            assert not rej.any() and (t[:, 3] == 1).all(), name
            hit = False
            for ph in (0, 1):
                es = [e for e in its if e["phase"] == ph]
                third = [i for i, e in enumerate(es) if e["stall"] < 1][2:3]
                hit = hit or bool(third and third[0] + 1 < len(es))
            assert hit, name
        elif tag == "all_gated":              # every edge gated, every solve succeeds, chi2 ends in noise; some trials of the second optimize() are decidable
            k = LC.decidable_rows(case, t)
            assert case["kind"] == "nav" and case.get("noise_tail") and base["its_first"] == 5 and (t[:, 3] == 1).all(), name
            assert base["erase"].all() and base["chi2_final"] < LC.NOISE_CHI2 and (t[:k, 0] == 1).sum() >= 2 and k < len(t), name
            assert not rej[:k].any(), name
        elif tag == "failed_solve_qmax":
            assert (base["its_first"], base["its_second"]) == (5, 1), name
            last = t[t[:, 0] == 1]
            assert len(last) == 10 and (last[:, 3] == 0).all() and list(last[:, 2]) == list(range(10)) and np.isneginf(last[:, 4]).all(), name
            assert (t[t[:, 0] == 0][:, 3] == 1).all() and base["chi2_final"] == 0 and base["erase"].all(), name
        elif tag == "mid_reject_retry":
            assert rej.any() and (t[:, 3] == 1).all(), name
            for i in np.flatnonzero(rej):     # every rejected trial is retried in the same iteration, and none is in the solve's last iteration
                assert i + 1 < len(t) and tuple(t[i + 1, :2]) == tuple(t[i, :2]) and t[i + 1, 2] == t[i, 2] + 1, name
                assert tuple(t[i, :2]) != tuple(t[-1, :2]), name
            seen.setdefault("mid", []).append((case["kind"], max(e["n"] for e in its), bool((rej & (t[:, 0] == 0)).any())))
        elif tag == "late_reject":
            assert rej.any() and (t[rej, 0] == 1).all() and (t[rej, 1] == base["its_second"] - 1).all() and base["its_second"] == 10, name
        elif tag == "plain":
            assert (base["its_first"], base["its_second"]) == (5, 10) and len(t) == 15 and not rej.any(), name
    mid = seen["mid"]
    assert any(n >= 3 for _, n, _ in mid) and any(p0 for _, _, p0 in mid)
