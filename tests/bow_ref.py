"""Literal pure-Python restatement of ORBmatcher::SearchByBoW(KeyFrame, Frame), shared by tests/test_oracle_bow.py and the hand-built cases
of tests/kf_matcher_cases.py. rule=None is the reference behaviour; a rule name alters ONE decision, only to prove on the CPU that a case
decides it (see tests/kf_matcher_ref.py)."""
import numpy as np
from kf_matcher_ref import ham, three_maxima, rotation_bin, TH_LOW, HISTO_LENGTH

BOW_RULES = ("tie_last", "th_low_exclusive", "ratio_le", "second_ignores_equal", "ignore_has_point", "not_exclusive")


def literal_search(kd, ka, kn, kh, fd, fa, fn, ratio, ori, rule=None):
    assert rule is None or rule in BOW_RULES, rule
    nF = len(fd); match = [-1] * nF; hist = [[] for _ in range(HISTO_LENGTH)]; nm = 0
    nodes = sorted(set(int(x) for x in kn if x >= 0) & set(int(x) for x in fn if x >= 0))
    for nd in nodes:
        for i in np.nonzero(kn == nd)[0]:
            if not kh[i] and rule != "ignore_has_point":
                continue
            b1, b2, bi = 256, 256, -1
            for j in np.nonzero(fn == nd)[0]:
                if match[j] >= 0 and rule != "not_exclusive":
                    continue
                d = ham(kd[i], fd[j])
                if d < b1 or (rule == "tie_last" and d == b1):
                    b2, b1, bi = b1, d, j
                elif d < b2 and not (rule == "second_ignores_equal" and d == b1):
                    b2 = d
            r1, r2 = np.float32(b1), np.float32(np.float32(ratio) * np.float32(b2))
            if (b1 < TH_LOW or (b1 == TH_LOW and rule != "th_low_exclusive")) and (r1 < r2 or (rule == "ratio_le" and r1 == r2)):
                if match[bi] >= 0:                         # (not_exclusive only) the earlier taker is displaced, as vpMapPointMatches[bestIdxF] = pMP would
                    nm -= 1
                    for h in hist:
                        if bi in h:
                            h.remove(bi)
                match[bi] = int(i); nm += 1
                if ori:
                    hist[rotation_bin(ka[i], fa[bi])].append(bi)
    if ori:
        keep = three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for j in hist[b]:
                    match[j] = -1; nm -= 1
    return nm, np.array(match, np.int32)
