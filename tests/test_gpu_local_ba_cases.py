"""The window solves (csrc/local_ba.hip) off the straight road: every fixture of tests/local_ba_cases.py — early stops by the stall rule,
restarts, failed factorisations retried to qmax == 10, a window that loses every edge while its solves succeed, rejected trials in mid-solve
and in the last iteration — against the CPU oracle,
through both drivers of the one Levenberg decision (csrc/lba_ctl.h): the single call (slots of trials enqueued ahead, the decision in the
last block of k_ba_f_errors_decide, restore and retry in the next slot) and the lock-step batch (k_bab_decide / k_bab_restore /
k_bab_phase). tests/test_local_ba_cases.py proves on the oracle alone that the fixtures take these paths and that none of their decisions
sits on a jump.

Bars: those of test_local_ba_matches_oracle — iteration counts equal, chi2 within 1e-5 relative, erase flags equal, key-frame states
within 1e-7, points within 1e-6 (1e-5 for the vision-only window) — and info[4] / info[5] equal to the oracle's numbers of trials and
of rejected trials. Where the oracle's chi2 is below 1e-12 (0 after a failed_solve_qmax window lost all its edges, 1e-25 after the
all_gated one did) a relative bar means nothing: there the device's value must not exceed 1e-12. The all_gated fixture ends in rounding
noise, so its second iteration count and its trial counts are not compared (check_against_oracle says what is)."""
import numpy as np
import pytest

import local_ba_cases as LC

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in LC.CASES]

# Mixed lists per kind (a batch entry point takes one kind of window), every tag of the kind beside the plain window, in two orders. In both
# orders window 4 rejects trials and window 5 stops early: at max_in_flight 5 they are the last of one lock-step group and the first of the next.
ORDERS = {
    ("nav", "a"): ["nav_plain_13", "nav_mid_122", "nav_stall_32", "nav_late_4", "nav_mid_131", "nav_restart_32", "nav_mid_126", "nav_stall_reset_223", "nav_all_gated_34"],
    ("nav", "b"): ["nav_stall_reset_223", "nav_all_gated_34", "nav_restart_32", "nav_plain_13", "nav_mid_131", "nav_stall_32", "nav_late_4", "nav_mid_122", "nav_mid_126"],
    ("se3", "a"): ["se3_plain_2", "se3_failed_42", "se3_stall_44", "se3_mid_153", "se3_mid_126", "se3_restart_40", "se3_failed_45", "se3_restart_44"],
    ("se3", "b"): ["se3_restart_44", "se3_mid_126", "se3_failed_45", "se3_plain_2", "se3_mid_153", "se3_stall_44", "se3_restart_40", "se3_failed_42"],
}


@pytest.fixture(scope="module")
def refs(oracle):
    """name -> (case, solver arguments, oracle result): computed once for the module, never written to."""
    out = {}
    for case in LC.CASES:
        args = LC.build(case, oracle)
        out[case["name"]] = (case, args, LC.solve_oracle(oracle, case["kind"], args))
    return out


def _chi2_close(got, ref):
    if ref < 1e-12:                      # 0 or rounding noise in the oracle: no relative bar; the device must be as small
        return got <= 1e-12
    return abs(got - ref) <= 1e-5 * ref


def check_against_oracle(name, got, ref, case):
    kind, tail = case["kind"], bool(case.get("noise_tail"))
    g = lambda k: got[k].item() if isinstance(got[k], np.ndarray) and got[k].ndim == 0 else got[k]
    print("%s: its %d+%d (oracle %d+%d) trials %d rejected %d (oracle %d, %d) chi2 %.9g (oracle %.9g)" % (
        name, g("its_first"), g("its_second"), ref["its_first"], ref["its_second"], g("n_trials"), g("n_rejected"), ref["n_trials"], ref["n_rejected"],
        g("chi2_final"), ref["chi2_final"]))
    assert int(g("its_first")) == ref["its_first"], name
    if tail:
        # a noise_tail fixture (all_gated): the second optimize() ends in rounding noise, where the number of iterations, trials and rejections
        # is not decidable (tests/local_ba_cases.py). The device must still run every trial the oracle's decidable rows hold, get to the
        # same noise (the chi2 bar below 1e-12) and, by the bars on states, points and erase flags, to the same solution
        k = LC.decidable_rows(case, ref["trials"])
        assert int(g("n_trials")) >= k and int(g("its_second")) >= int((ref["trials"][:k, 0] == 1).sum()), name
        assert ref["chi2_final"] < LC.NOISE_CHI2, name
    else:
        assert int(g("its_second")) == ref["its_second"], name
        assert (int(g("n_trials")), int(g("n_rejected"))) == (ref["n_trials"], ref["n_rejected"]), name
    assert _chi2_close(float(g("chi2_first")), ref["chi2_first"]), (name, g("chi2_first"), ref["chi2_first"])
    assert _chi2_close(float(g("chi2_final")), ref["chi2_final"]), (name, g("chi2_final"), ref["chi2_final"])
    assert np.array_equal(got["erase"], ref["erase"]), name
    np.testing.assert_allclose(got["kfs"], ref["kfs"], rtol=0, atol=1e-7, err_msg=name)
    np.testing.assert_allclose(got["points"], ref["points"], rtol=0, atol=1e-6 if kind == "nav" else 1e-5, err_msg=name)


def _solve_single(kind, args):
    from viorb_amd import LocalBundleAdjustment, LocalBundleAdjustmentNavState
    return LocalBundleAdjustmentNavState(**args) if kind == "nav" else LocalBundleAdjustment(**args)


def _solve_batch(kind, problems, max_in_flight):
    from viorb_amd import LocalBundleAdjustmentBatch, LocalBundleAdjustmentNavStateBatch
    return (LocalBundleAdjustmentNavStateBatch if kind == "nav" else LocalBundleAdjustmentBatch)(problems, max_in_flight=max_in_flight)


@pytest.mark.parametrize("name", NAMES)
def test_single_call_matches_oracle(refs, name):
    """The single call never leaves the device path: the host enqueues as many trial slots as the phase has iterations, the last block of
    k_ba_f_errors_decide takes every decision (lba_decide), and after a rejected trial the next slot restores and retries without
    linearising. mid_reject_retry: retries inside a chunk; late_reject: slots beyond the phase's 10th; failed_solve_qmax: ten trials of
    one iteration, so the retry count and the restore flag cross a chunk boundary; stall_stop, restart, stall_reset, all_gated: the end
    of a phase is decided on the device while slots are still queued. Either kind of window."""
    case, args, ref = refs[name]
    check_against_oracle(name, _solve_single(case["kind"], args), ref, case)


@pytest.mark.parametrize("kind", ["nav", "se3"])
def test_single_call_equals_its_lockstep_group(refs, kind):
    """One rule, two drivers: every window of the mixed list solved by a single call and by the lock-step batch (one group of 16) takes the
    same iterations, trials and rejections, gates the same edges and ends in the same state to the 1e-9 of
    test_local_ba_batch_equals_single_calls (the Schur sums' order differs between two runs). The noise_tail fixture's undecidable fields
    are skipped as check_against_oracle skips them."""
    names = ORDERS[(kind, "a")]
    batch = _solve_batch(kind, [refs[n][1] for n in names], 16)
    assert len(batch) == len(names)
    for n, b in zip(names, batch):
        case, args, _ = refs[n]
        s = _solve_single(kind, args)
        print("%s: single %d+%d trials %d rejected %d, batch %d+%d trials %d rejected %d; max |d kfs| %.3g |d points| %.3g chi2 %.17g / %.17g" % (
            n, s["its_first"], s["its_second"], s["n_trials"], s["n_rejected"], b["its_first"], b["its_second"], b["n_trials"], b["n_rejected"],
            np.abs(s["kfs"] - b["kfs"]).max(), np.abs(s["points"] - b["points"]).max(), s["chi2_final"], b["chi2_final"]))
        assert s["its_first"] == b["its_first"], n
        if not case.get("noise_tail"):
            assert (s["its_second"], s["n_trials"], s["n_rejected"]) == (b["its_second"], b["n_trials"], b["n_rejected"]), n
        np.testing.assert_array_equal(s["erase"], b["erase"], err_msg=n)
        np.testing.assert_allclose(s["kfs"], b["kfs"], rtol=0, atol=1e-9, err_msg=n)
        np.testing.assert_allclose(s["points"], b["points"], rtol=0, atol=1e-9, err_msg=n)
        if b["chi2_final"] < 1e-12:          # 0 or rounding noise (_chi2_close): no relative bar, both must be as small
            assert s["chi2_final"] <= 1e-12, (n, s["chi2_final"], b["chi2_final"])
        else:
            assert abs(s["chi2_final"] - b["chi2_final"]) <= 1e-9 * b["chi2_final"], (n, s["chi2_final"], b["chi2_final"])


@pytest.mark.parametrize("max_in_flight", [1, 4, 5, 16])
@pytest.mark.parametrize("order", ["a", "b"])
@pytest.mark.parametrize("kind", ["nav", "se3"])
def test_lockstep_mixed_batch_matches_oracle(refs, kind, order, max_in_flight):
    """Windows that reject, retry, fail to factorise, stop early and run the full 5 + 10 advance in one lock-step group, and every one of
    them equals the oracle — not merely its own single call. This fails if a window's restore (k_bab_restore), retry count (BA_B_QMAX) or
    phase flags leak to a neighbour of its group, if a retry re-linearises, or if a finished window is touched again."""
    names = ORDERS[(kind, order)]
    got = _solve_batch(kind, [refs[n][1] for n in names], max_in_flight)
    assert len(got) == len(names)
    for n, g in zip(names, got):
        check_against_oracle(n, g, refs[n][2], refs[n][0])


@pytest.mark.parametrize("kind,stopped", [("nav", "nav_stall_32"), ("se3", "se3_mid_153")])
def test_lockstep_mixed_batch_with_a_stop_flag_set_before_the_call(refs, kind, stopped):
    """One window's pbStopFlag is up before the call: it comes back untouched (inputs copied, no iteration, no trial), and its neighbours —
    the rejecting ones included — still equal the oracle."""
    names = ORDERS[(kind, "a")]
    probs = [dict(refs[n][1], stop=np.ones(1, np.int32)) if n == stopped else refs[n][1] for n in names]
    got = _solve_batch(kind, probs, 16)
    for n, g in zip(names, got):
        if n != stopped:
            check_against_oracle(n, g, refs[n][2], refs[n][0])
            continue
        a = refs[n][1]
        np.testing.assert_array_equal(g["kfs"], a["kfs"][:a["n_local"]])
        np.testing.assert_array_equal(g["points"], a["points"])
        assert g["erase"].sum() == 0 and (g["its_first"], g["its_second"], g["n_trials"], g["n_rejected"]) == (0, 0, 0, 0)
