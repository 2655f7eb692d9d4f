"""Scenes for Tracking::UpdateLocalMap (tests/test_local_map_ref.py, tests/test_gpu_local_map.py): hand-built ones, the smallest shapes
at which the routine can go wrong, each with the outputs it must give written out by hand (`want`, checked against the checker
tests/local_map_ref.py before anything else is), the limit scenes, sized scenes for the kernels' chunk edges, broken snapshots and a
random generator. CASES: (name, scene, caps, want)."""
import numpy as np
from viorb_amd import local_map as M
import local_map_ref as T


def kf(pts=(), **k):
    return dict(pts=list(pts), **k)


def pt(*obs, bad=False):
    return dict(obs=list(obs), bad=bad)


def _cases():
    C = []
    add = lambda name, scene, want, **caps: C.append((name, scene, caps, want))
    # no votes: the frame holds a bad point and a point nobody observes. The previous list and reference stay; the points are rebuilt from that list
    add("no_votes", M.scene_from_lists([kf([1, 3, -1]), kf([0]), kf([2, 1])], [pt(0, bad=True), pt(), pt(2), pt(bad=True)], [0, 1], prev_lkf=[2, 0], prev_ref=2),
        dict(status=T.NO_VOTES, lkf=[2, 0], n_voted=0, ref_kf=2, lpt=[2, 1], frame_point_out=[-1, 1], kf_votes=[0, 0, 0]))
    add("empty_frame", M.scene_from_lists([kf([0]), kf([0, 1])], [pt(0, 1), pt(1)], [], prev_lkf=[1], prev_ref=-1),
        dict(status=T.NO_VOTES, lkf=[1], ref_kf=-1, lpt=[0, 1], frame_point_out=[]))
    # every voted key frame is bad: the list is cleared and ends empty, the reference key frame is kept
    add("all_voted_bad", M.scene_from_lists([kf([0], bad=True), kf([0], bad=True)], [pt(0, 1)], [0], prev_lkf=[1], prev_ref=1),
        dict(status=T.OK, lkf=[], n_voted=0, ref_kf=1, lpt=[], kf_votes=[1, 1]))
    # a tie of two votes each between slots 0 and 2; pointer order is 2, 0, 1: slot 2 is walked first and wins; slot order would give 0
    add("tie_first_in_key_order", M.scene_from_lists([kf([0]), kf([2]), kf([1])], [pt(0, 2), pt(0, 2), pt(1)], [0, 1, 2], by_key=[2, 0, 1]),
        dict(status=T.OK, lkf=[2, 0, 1], n_voted=3, ref_kf=2, lpt=[1, 0, 2], kf_votes=[2, 1, 2]))
    # a later key frame with strictly more votes takes over; an equal one does not
    add("strictly_more_wins", M.scene_from_lists([kf(), kf(), kf()], [pt(0, 1, 2), pt(1, 2), pt(2)], [0, 1, 2]),
        dict(lkf=[0, 1, 2], ref_kf=2, kf_votes=[1, 2, 3]))
    # a bad frame point is cleared and does not vote; point 0 sits on two keypoints and votes twice
    add("bad_point_cleared_and_double_vote", M.scene_from_lists([kf([0]), kf([1])], [pt(0), pt(1, bad=True)], [0, 1, 0, -1]),
        dict(status=T.OK, lkf=[0], ref_kf=0, lpt=[0], frame_point_out=[0, -1, 0, -1], kf_votes=[2, 0]))
    # votes for the bad key frame 1 are counted (3, the most), but the walk skips it: it is neither listed nor the reference
    add("votes_to_bad_key_frame", M.scene_from_lists([kf([0]), kf([1], bad=True), kf([2])], [pt(0, 1), pt(1), pt(1, 2)], [0, 1, 2]),
        dict(status=T.OK, lkf=[0, 2], n_voted=2, ref_kf=0, lpt=[0, 2], kf_votes=[1, 3, 1]))
    # neighbours of 0: 1 is bad, 2 is in the list already, 3 is taken, 4 is not (one per key frame). 3 was added by the loop: it is not
    # visited, so its neighbour 5 stays out
    add("neighbour_choice", M.scene_from_lists([kf([0], covis=[1, 2, 3, 4]), kf(bad=True), kf([0]), kf(covis=[5]), kf(), kf()], [pt(0, 2)], [0]),
        dict(status=T.OK, lkf=[0, 2, 3], n_voted=2, ref_kf=0, kf_votes=[1, 0, 1, 0, 0, 0]))
    # children in the given order 2, 3, 1: 2 is bad, 3 is taken, 1 is not
    add("child_choice", M.scene_from_lists([kf([0], children=[2, 3, 1]), kf(), kf(bad=True), kf()], [pt(0)], [0]),
        dict(lkf=[0, 3], n_voted=1))
    # parent, prev and next get no bad test
    add("bad_parent_prev_next_added", M.scene_from_lists([kf([0], parent=1, prev=2, next=3), kf(bad=True), kf(bad=True), kf(bad=True)], [pt(0)], [0]),
        dict(lkf=[0, 1, 2, 3], n_voted=1))
    add("parent_equals_prev", M.scene_from_lists([kf([0], parent=1, prev=1, next=2), kf(), kf()], [pt(0)], [0]),
        dict(lkf=[0, 1, 2], n_voted=1))
    # the order inside one iteration: neighbour, child, parent, prev, next
    add("order_of_one_iteration", M.scene_from_lists([kf([0], covis=[5], children=[4], parent=3, prev=2, next=1), kf(), kf(), kf(), kf(), kf()], [pt(0)], [0]),
        dict(lkf=[0, 5, 4, 3, 2, 1]))
    # the second voted key frame finds its neighbour already taken by the first one's iteration and takes the next
    add("marks_from_earlier_iterations", M.scene_from_lists([kf([0], covis=[2]), kf([0], covis=[2, 3]), kf(), kf()], [pt(0, 1)], [0]),
        dict(lkf=[0, 1, 2, 3], n_voted=2))
    # points shared by several key frames stay at their first position; null and bad entries are dropped; key frame 1 has no keypoints
    add("points_first_position", M.scene_from_lists([kf([0, 1, -1, 2, 1]), kf(), kf([1, 3, 0, 2])], [pt(0, 2), pt(), pt(bad=True), pt(2), pt(1)], [0, 3, 4]),
        dict(status=T.OK, lkf=[0, 1, 2], lpt=[0, 1, 3], n_lpt=3, kf_votes=[1, 1, 2], ref_kf=2))
    # one more local key frame than lcap, one more local point than pcap
    add("lcap_overflow_by_one", M.scene_from_lists([kf([0], parent=1, prev=2, next=3), kf(), kf(), kf()], [pt(0)], [0]),
        dict(status=T.OVERFLOW, n_lkf=4, n_lpt=1), lcap=3)
    add("lcap_exact", M.scene_from_lists([kf([0], parent=1, prev=2, next=3), kf(), kf(), kf()], [pt(0)], [0]), dict(status=T.OK, lkf=[0, 1, 2, 3]), lcap=4)
    add("pcap_overflow_by_one", M.scene_from_lists([kf([0, 1, 2])], [pt(0), pt(), pt()], [0]), dict(status=T.OVERFLOW, n_lkf=1, n_lpt=3), pcap=2)
    add("pcap_exact", M.scene_from_lists([kf([0, 1, 2])], [pt(0), pt(), pt()], [0]), dict(status=T.OK, lpt=[0, 1, 2]), pcap=3)
    add("no_key_frames", M.scene_from_lists([], [], []), dict(status=T.NO_VOTES, n_lkf=0, n_lpt=0, ref_kf=-1))
    for n, size in ((75, 81), (79, 84), (80, 85), (81, 81), (82, 82)):
        add("limit_%d_voted" % n, limit_scene(n), dict(status=T.OK, n_voted=n, n_lkf=size, ref_kf=0))
    return C


def limit_scene(n):
    """n voted key frames (slots 0 .. n-1, one vote each) and six more: slot 0 can add five of them in its iteration (neighbour, child,
    parent, prev, next), slot 1 the sixth. 75: 80 after the first iteration, which is not more than 80, so the second runs and adds one, 81;
    79 and 80: one iteration takes the list to 84 and 85 and the loop breaks; 81 and 82: the break comes before the first iteration."""
    kfs = [kf([k]) for k in range(n)] + [kf([n + e]) for e in range(6)]
    kfs[0].update(covis=[n], children=[n + 1], parent=n + 2, prev=n + 3, next=n + 4)
    kfs[1].update(covis=[n + 5])
    return M.scene_from_lists(kfs, [pt(k) for k in range(n)] + [pt() for _ in range(6)], list(range(n)))


def sized_scene(seed, nk, nkp, n_frame, n_pt=150):
    """nk key frames, the first two of them with nkp keypoints each (the rest with up to 3), a frame of n_frame keypoints: for the edges of
    the kernels' strides and chunks. Points repeat within and between the tables."""
    rng = np.random.default_rng(seed)
    pts = [pt(*rng.choice(nk, size=min(nk, int(rng.integers(0, 4))), replace=False).tolist(), bad=bool(rng.random() < 0.1)) for _ in range(n_pt)]
    table = lambda n: [int(p) if rng.random() < 0.9 else -1 for p in rng.integers(0, n_pt, n)]
    kfs = [kf(table(nkp if k < 2 else int(rng.integers(0, 4))), bad=bool(k >= 2 and rng.random() < 0.1)) for k in range(nk)]
    for k in range(nk):
        kfs[k].update(covis=rng.choice(nk, size=min(nk, 3), replace=False).tolist(), prev=k - 1, next=k + 1 if k + 1 < nk else -1, parent=int(rng.integers(-1, nk)))
    pts[0], pts[1] = pt(0, 1), pt(1, 0)                              # the two large tables are always voted
    frame = [0, 1] + [int(p) for p in rng.integers(-1, n_pt, max(n_frame - 2, 0))]
    return M.scene_from_lists(kfs, pts, frame[:max(n_frame, 2)], by_key=rng.permutation(nk).tolist())


def loop_scene(seed, nk, n_voted=12):
    """nk key frames of which only n_voted are voted, so the neighbour loop runs and adds neighbours, children and links from all over the
    slot range: with nk above the LDS limit its marks and list entries live in the workspace."""
    rng = np.random.default_rng(seed)
    voted = rng.choice(nk, n_voted, replace=False)
    n_pt = 60                                                        # the first 30 are observed (by one to three voted key frames) and held by the frame
    pts = [pt(*rng.choice(voted, size=int(rng.integers(1, 4)), replace=False).tolist()) if p < 30 else pt(bad=bool(rng.random() < 0.2)) for p in range(n_pt)]
    kfs = []
    for k in range(nk):
        link = lambda: int(rng.integers(0, nk)) if rng.random() < 0.8 else -1
        kfs.append(kf([int(p) for p in rng.integers(-1, n_pt, int(rng.integers(0, 4)))], bad=bool(rng.random() < 0.15), parent=link(), prev=link(), next=link(),
                      covis=rng.choice(nk, size=10, replace=False).tolist(), children=rng.choice(nk, size=int(rng.integers(0, 4)), replace=False).tolist()))
    return M.scene_from_lists(kfs, pts, list(range(30)), by_key=rng.permutation(nk).tolist())


def sized_scenes():
    """(name, scene): keypoint, frame and key-frame counts at shape +- 1 around every stride and chunk that viorb_update_local_map_shape
    reports, a child list one longer than the wavefront, and the neighbour loop at and above the LDS limit of the key-frame count."""
    thr, chunk, wave, lds_kf = M.shape()
    out = []
    for i, v in enumerate(sorted({wave, thr, chunk})):
        for d in (-1, 0, 1):
            out.append(("kp_%d" % (v + d), sized_scene(10 * i + d + 1, 5, v + d, 40)))              # entries of one key frame, and of the list: 2 (v + d) + a few
            out.append(("frame_%d" % (v + d), sized_scene(100 + 10 * i + d + 1, 6, 7, v + d)))
    for v in (thr, lds_kf):
        for d in (-1, 0, 1):
            out.append(("kf_%d" % (v + d), sized_scene(200 + v + d, v + d, 9, 700, n_pt=900)))
    for d in (0, 1):
        out.append(("loop_kf_%d" % (lds_kf + d), loop_scene(300 + d, lds_kf + d)))
    out.append(("children_%d" % (wave + 1), M.scene_from_lists([kf([0], children=list(range(1, wave + 2)))] + [kf(bad=True) for _ in range(wave)] + [kf()], [pt(0)], [0])))
    return out


def random_scene(rng, max_kf=40, max_kp=64, max_pt=200):
    """A random stream: at most max_kf key frames, max_kp keypoints each and max_pt points; now and then no key frames, an empty frame, a
    frame of bad points only."""
    nk = 0 if rng.random() < 0.03 else int(rng.integers(1, max_kf + 1))
    n_pt = int(rng.integers(0, max_pt + 1)) if nk else 0
    p_bad = rng.choice([0.0, 0.1, 0.5])
    pts = [pt(*rng.choice(nk, size=min(nk, int(rng.integers(0, 7))), replace=False).tolist(), bad=bool(rng.random() < p_bad)) for _ in range(n_pt)]
    kfs = []
    for k in range(nk):
        n = int(rng.integers(0, max_kp + 1)) if n_pt else 0
        tab = [int(p) if rng.random() < 0.8 else -1 for p in rng.integers(0, max(n_pt, 1), n)]
        link = lambda: int(rng.integers(0, nk)) if rng.random() < 0.7 else -1
        kfs.append(kf(tab, bad=bool(rng.random() < 0.15), parent=link(), prev=link(), next=link(),
                      covis=rng.choice(nk, size=min(nk, int(rng.integers(0, 11))), replace=False).tolist(),
                      children=rng.choice(nk, size=min(nk, int(rng.integers(0, 5))), replace=False).tolist()))
    mode = rng.random()
    n_frame = 0 if mode < 0.05 or not n_pt else int(rng.integers(1, 65))
    frame = [int(p) if rng.random() < 0.7 else -1 for p in rng.integers(0, max(n_pt, 1), n_frame)]
    if 0.05 <= mode < 0.1:
        frame = [p for p in frame if p < 0 or pts[p]["bad"] or not pts[p]["obs"]]
    prev = rng.choice(nk, size=int(rng.integers(0, nk + 1)), replace=False).tolist() if nk else []
    return M.scene_from_lists(kfs, pts, frame, by_key=rng.permutation(nk).tolist(), prev_lkf=prev, prev_ref=int(rng.integers(-1, nk)) if nk else -1)


_RANDOM = {}


def random_streams(seed=11, n=300):
    """n random streams and the checker's outputs, computed once and shared (nobody changes them)."""
    if (seed, n) not in _RANDOM:
        rng = np.random.default_rng(seed)
        scenes = [random_scene(rng) for _ in range(n)]
        _RANDOM[(seed, n)] = (scenes, [T.update_local_map(s) for s in scenes])
    return _RANDOM[(seed, n)]


def broken(scene):
    """(what, scene) for every kind of broken snapshot the validator refuses, made from a scene with at least 3 key frames, a child, an
    observation, a keypoint with a point, a frame keypoint and a previous list of at least 2."""
    nk, n_pt = len(scene["kf_bad"]), len(scene["pt_bad"])
    out = []

    def brk(what, field, index, value):
        s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
        if index is None:
            s[field] = value
        else:
            s[field][index] = value
        out.append((what, s))
    brk("a point index at the end of the stream", "kp_point", int(np.argmax(scene["kp_point"] >= 0)), n_pt)
    brk("a point index below -1", "kp_point", 0, -2)
    brk("a frame point past the end", "frame_point", 0, n_pt + 5)
    brk("an observation slot at the end", "obs", 0, nk)
    brk("descending keypoint offsets", "kp_start", 1, int(scene["kp_start"][2]) + 1)
    brk("a negative observation offset", "obs_start", 1, -4)
    brk("a child offset past the total", "child_start", 1, 1 << 28)
    brk("a child slot past the end", "child_kf", 0, nk)
    brk("a parent outside the snapshot", "kf_parent", 1, nk)
    brk("a prev below -1", "kf_prev", 0, -2)
    brk("a next outside the snapshot", "kf_next", 2, 1 << 20)
    brk("a neighbour outside the snapshot", "covis10", (1, 3), nk)
    brk("kf_by_key with a slot twice", "kf_by_key", 0, int(scene["kf_by_key"][1]))
    brk("kf_by_key with a slot out of range", "kf_by_key", 1, nk)
    brk("prev_lkf with a slot out of range", "prev_lkf", 0, -1)
    brk("prev_lkf with a slot twice", "prev_lkf", 0, int(scene["prev_lkf"][1]))
    brk("prev_ref_kf out of range", "prev_ref", None, nk)
    return out


def breakable_scene():
    return M.scene_from_lists([kf([0, 1], children=[1, 2], covis=[1]), kf([1, 2], parent=0, prev=0, next=2), kf([2, -1], parent=0, prev=1)],
                              [pt(0), pt(0, 1), pt(1, 2)], [1, 2, -1], by_key=[1, 2, 0], prev_lkf=[2, 1], prev_ref=2)


CASES = _cases()


def expected(name):
    _, scene, caps, _ = next(c for c in CASES if c[0] == name)
    return T.update_local_map(scene, lcap=caps.get("lcap"), pcap=caps.get("pcap"))
