"""Seeded synthetic inputs for tests and bench: no dataset is available, so images
are band-limited noise plus random filled rectangles/discs, and consecutive frames of a stream are
the same scene under a small similarity warp. numpy/scipy only; no GPU, no oracle."""
import numpy as np
from scipy import ndimage

EUROC_K = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375)   # reference Examples/ROS/ORB_VIO/launch/euroc.yaml
EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.762e-05, 0.0)   # Camera.k1 k2 p1 p2 (euroc.yaml:64-67), k3 = 0


def make_image(seed, w=752, h=480, n_shapes=None):
    """u8 [h, w] image: Gaussian-filtered white noise (sigma 3 px, +-40 around 128) + 400..1500
    random filled rectangles/discs with uniform grey levels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    noise = ndimage.gaussian_filter(rng.standard_normal((h, w)), 3.0)
    noise = noise / (np.abs(noise).max() + 1e-12) * 40.0
    img = 128.0 + noise
    if n_shapes is None:
        n_shapes = int(rng.integers(400, 1500))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_shapes):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        g = rng.uniform(20, 235)
        if rng.random() < 0.5:
            hw, hh = rng.uniform(3, 40), rng.uniform(3, 40)
            x0, x1 = int(max(cx - hw, 0)), int(min(cx + hw, w))
            y0, y1 = int(max(cy - hh, 0)), int(min(cy + hh, h))
            img[y0:y1, x0:x1] = g
        else:
            r = rng.uniform(3, 30)
            x0, x1 = int(max(cx - r, 0)), int(min(cx + r + 1, w))
            y0, y1 = int(max(cy - r, 0)), int(min(cy + r + 1, h))
            m = (xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2 <= r * r
            img[y0:y1, x0:x1][m] = g
    img += rng.normal(0, 1.5, size=img.shape)          # sensor-like noise so flat areas are not exact ties
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def warp_image(img, dx, dy, roll_deg, seed=0):
    """Same scene moved by (dx, dy) px and rolled by roll_deg about the image centre (bilinear)."""
    h, w = img.shape
    a = np.deg2rad(roll_deg)
    c, s = np.cos(a), np.sin(a)
    R = np.array([[c, -s], [s, c]])                    # output (y,x) -> input (y,x) rotation
    centre = np.array([h / 2.0, w / 2.0])
    offset = centre - R @ centre - np.array([dy, dx])
    out = ndimage.affine_transform(img.astype(np.float32), R, offset=offset, order=1, mode="reflect")
    rng = np.random.Generator(np.random.PCG64(seed + 7919))
    out += rng.normal(0, 1.0, size=out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def make_stream(seed, n_frames, w=752, h=480):
    """A short synthetic camera stream: frame k = base scene warped by a smooth small motion."""
    base = make_image(seed, w, h)
    rng = np.random.Generator(np.random.PCG64(seed + 104729))
    frames, motions = [], []
    dx = dy = roll = 0.0
    for k in range(n_frames):
        frames.append(base if k == 0 else warp_image(base, dx, dy, roll, seed=seed * 1000 + k))
        motions.append((dx, dy, roll))
        dx += rng.uniform(-4, 4); dy += rng.uniform(-3, 3); roll += rng.uniform(-0.7, 0.7)
        dx, dy, roll = np.clip(dx, -10, 10), np.clip(dy, -10, 10), np.clip(roll, -3, 3)
    return frames, motions


# ==================================================================================================
# Synthetic visual-inertial problems: one "last frame -> current frame" step.
# Flat layouts (shared with include/viorb.h):
#   navstate[22] = P3 V3 q4(x,y,z,w) bg3 ba3 dbg3 dba3 ; cam[16] = fx fy cx cy Rbc9 Pbc3
#   obs[n,6] = Pw3 u v invSigma2 ; imu[n,7] = gyro3 acc3 t
# ==================================================================================================
EUROC_TBC = np.array([[0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975],
                      [0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768],
                      [-0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949],
                      [0.0, 0.0, 0.0, 1.0]])       # reference Examples/ROS/ORB_VIO/launch/euroc.yaml Camera.Tbc
GRAVITY_W = np.array([0.0, 0.0, -9.81])


def _rotvec_to_R(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _R_to_quat(R):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()           # x, y, z, w
    return q if q[3] >= 0 else -q


def euroc_cam():
    R = EUROC_TBC[:3, :3]
    u, _, vt = np.linalg.svd(R)                     # yaml values are 12-digit: re-orthonormalise
    R = u @ vt
    return np.concatenate([[EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"]], R.ravel(), EUROC_TBC[:3, 3]])


def navstate(P, V, R, bg=(0, 0, 0), ba=(0, 0, 0)):
    return np.concatenate([P, V, _R_to_quat(R), bg, ba, np.zeros(3), np.zeros(3)]).astype(np.float64)


def make_vio_problem(seed, n_points=300, outlier_frac=0.05, n_imu=10, w=752, h=480, pix_sigma=1.0):
    """One tracking step with ground truth: last frame at t0, current frame at t0 + n_imu*5 ms."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = euroc_cam()
    fx, fy, cx, cy = cam[:4]
    Rbc, Pbc = cam[4:13].reshape(3, 3), cam[13:16]
    dt = 0.005
    T = n_imu * dt
    R0 = _rotvec_to_R(rng.normal(0, 0.4, 3))
    P0 = rng.normal(0, 1.0, 3)
    V0 = rng.normal(0, 0.5, 3)
    omega = rng.normal(0, 0.1, 3)                   # body rate, constant over the step
    a_w = rng.normal(0, 0.5, 3)                     # world acceleration, constant over the step
    bg = rng.normal(0, 0.002, 3)
    ba = rng.normal(0, 0.02, 3)
    t0 = 100.0 + seed * 0.05
    ts = t0 + dt * (np.arange(n_imu) + 0.3)         # IMU stamps are not aligned with the frame stamps
    imu = np.zeros((n_imu, 7))
    for k, t in enumerate(ts):
        Rt = R0 @ _rotvec_to_R(omega * (t - t0))
        imu[k, :3] = omega + bg + rng.normal(0, 1e-3, 3)
        imu[k, 3:6] = Rt.T @ (a_w - GRAVITY_W) + ba + rng.normal(0, 1e-2, 3)
        imu[k, 6] = t
    t1 = t0 + T
    R1 = R0 @ _rotvec_to_R(omega * T)
    P1 = P0 + V0 * T + 0.5 * a_w * T * T
    V1 = V0 + a_w * T

    def project(Rwb, Pwb, Pw):
        Pc = (Rbc.T @ (Rwb.T @ (Pw - Pwb).T)).T - Rbc.T @ Pbc
        return np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1), Pc[:, 2]

    # points seen from the current camera, then kept if also inside the last image
    uv = np.stack([rng.uniform(20, w - 20, 4 * n_points), rng.uniform(20, h - 20, 4 * n_points)], 1)
    z = rng.uniform(2, 10, len(uv))
    Pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    Pw = (R1 @ (Rbc @ (Pc + Rbc.T @ Pbc).T)).T + P1
    uv0, z0 = project(R0, P0, Pw)
    ok = (z0 > 0.5) & (uv0[:, 0] > 20) & (uv0[:, 0] < w - 20) & (uv0[:, 1] > 20) & (uv0[:, 1] < h - 20)
    Pw, uv, uv0 = Pw[ok][:n_points], uv[ok][:n_points], uv0[ok][:n_points]
    n = len(Pw)
    octave = rng.integers(0, 8, n)
    sig = (1.2 ** octave) * pix_sigma
    inv_sigma2 = (1.0 / (np.float32(1.2) ** octave).astype(np.float32) ** 2).astype(np.float64)

    def observe(uvt, salt):
        r = np.random.Generator(np.random.PCG64(seed * 7 + salt))
        o = uvt + r.normal(0, 1, uvt.shape) * sig[:, None]
        bad = r.random(n) < outlier_frac
        o[bad] += r.choice([-1, 1], (bad.sum(), 2)) * r.uniform(15, 25, (bad.sum(), 2))
        return np.float32(o).astype(np.float64), bad                       # keypoints are float32 in the reference

    oc, bad_c = observe(uv, 1)
    ol, bad_l = observe(uv0, 2)
    obs_cur = np.concatenate([Pw, oc, inv_sigma2[:, None]], 1)
    obs_last = np.concatenate([Pw, ol, inv_sigma2[:, None]], 1)
    ns_last_true = navstate(P0, V0, R0, bg, ba)
    ns_cur_true = navstate(P1, V1, R1, bg, ba)
    # what tracking would hold: last state slightly off, bias estimate slightly off
    ns_last = navstate(P0 + rng.normal(0, 0.01, 3), V0 + rng.normal(0, 0.02, 3), R0 @ _rotvec_to_R(rng.normal(0, 0.003, 3)),
                       bg + rng.normal(0, 2e-4, 3), ba + rng.normal(0, 5e-3, 3))
    prior_info = np.diag(np.concatenate([np.full(3, 1e4), np.full(3, 1e3), np.full(3, 1e5), np.full(3, 1e3)]))
    return dict(cam=cam, gw=GRAVITY_W.copy(), imu=imu, t_last=t0, t_cur=t1, ns_last=ns_last, ns_last_true=ns_last_true,
                ns_cur_true=ns_cur_true, obs_cur=obs_cur, obs_last=obs_last, outlier_cur_true=bad_c, outlier_last_true=bad_l,
                prior=ns_last.copy(), marg_cov_inv=prior_info, octave=octave)


# ==================================================================================================
# A full synthetic visual-inertial stream: a textured plane z = Z0 in the world frame (= the frame of
# the reference camera that sees `base` exactly), a smooth 6-DoF body trajectory, perspective-correct
# rendered frames, and IMU samples consistent with the trajectory.
# ==================================================================================================
PLANE_Z0 = 5.0
GRAVITY_CAM_WORLD = np.array([0.0, 9.81, 0.0])       # world = reference camera frame, y points down


_RAY_CACHE = {}


def pixel_rays(w, h, cam4, dist=None):
    """Normalised ray (x, y, 1) of every pixel of a w x h image for the pinhole intrinsics cam4 and, when given, the lens distortion
    (the inverse model run to convergence); cached per camera — every frame of a stream shares it."""
    key = (w, h, tuple(float(v) for v in cam4), None if dist is None else tuple(float(v) for v in dist))
    r = _RAY_CACHE.get(key)
    if r is None:
        fx, fy, cx, cy = cam4
        v, u = np.mgrid[0:h, 0:w].astype(np.float64)
        xn, yn = (u - cx) / fx, (v - cy) / fy
        if dist is not None and dist[0] != 0:
            xn, yn = undistort_normalized(xn, yn, dist)
        if len(_RAY_CACHE) > 8:
            _RAY_CACHE.clear()
        r = _RAY_CACHE[key] = (xn, yn)
    return r


def undistort_normalized(xd, yd, dist, iters=20):
    """Inverse of the radial-tangential model by fixed-point iteration run to convergence (the TRUE camera of the synthetic world;
    the reference's cv::undistortPoints stops after five iterations)."""
    k1, k2, p1, p2, k3 = [float(v) for v in dist]
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        ic = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x); dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (xd - dx) * ic; y = (yd - dy) * ic
    return x, y


def render_view(base, cam, Rcw, tcw, seed=0, noise=1.0, dist=None):
    """Image of the plane z = PLANE_Z0 (textured with `base` as seen from Tcw = I) from pose (Rcw, tcw). dist = k1 k2 p1 p2 k3: the
    camera has that lens distortion (pixel -> ray through the inverse model), as the EuRoC camera of the reference's settings file."""
    h, w = base.shape
    fx, fy, cx, cy = cam[:4]
    xn, yn = pixel_rays(w, h, cam[:4], dist)
    d = np.stack([xn, yn, np.ones_like(xn)], -1) @ Rcw          # Rcw^T d, row-vector form
    O = -Rcw.T @ tcw
    s = (PLANE_Z0 - O[2]) / d[..., 2]
    X = O[0] + s * d[..., 0]
    Y = O[1] + s * d[..., 1]
    ub = fx * X / PLANE_Z0 + cx
    vb = fy * Y / PLANE_Z0 + cy
    out = ndimage.map_coordinates(base.astype(np.float32), [vb, ub], order=1, mode="reflect")
    if noise > 0:
        out = out + np.random.Generator(np.random.PCG64(seed + 31337)).normal(0, noise, out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def cam_pose_from_navstate(ns, cam):
    """(Rcw, tcw) in float64 from a NavState and Tbc — Frame::UpdatePoseFromNS, reference src/Frame.cc:88-105."""
    from scipy.spatial.transform import Rotation
    Rwb = Rotation.from_quat(ns[6:10]).as_matrix()
    Rbc, Pbc = cam[4:13].reshape(3, 3), cam[13:16]
    Rcw = (Rwb @ Rbc).T
    Pwc = Rwb @ Pbc + ns[:3]
    return Rcw, -Rcw @ Pwc


def backproject_to_plane(uv, ns, cam):
    """World points on the plane z = PLANE_Z0 seen at pixels uv [n,2] from NavState ns."""
    Rcw, tcw = cam_pose_from_navstate(ns, cam)
    fx, fy, cx, cy = cam[:4]
    d = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], 1) @ Rcw
    O = -Rcw.T @ tcw
    s = (PLANE_Z0 - O[2]) / d[:, 2]
    return O[None, :] + s[:, None] * d


def make_vi_stream(seed, n_frames, w=752, h=480, n_imu=10, imu_dt=0.005):
    """Returns dict(frames [n,h,w] u8, ns_true [n,22], imu list of [n_imu,7] per interval (imu[k] spans
    frame k-1 -> k, imu[0] is None), t [n], cam[16], gw[3])."""
    rng = np.random.Generator(np.random.PCG64(seed + 424243))
    cam = euroc_cam()
    Rbc, Pbc = cam[4:13].reshape(3, 3), cam[13:16]
    base = make_image(seed, w, h)
    # body pose such that the camera starts at Tcw = I:  Rwb = Rbc^T, Pwb = -Rwb Pbc
    R = Rbc.T.copy(); P = -R @ Pbc
    V = rng.normal(0, 0.3, 3) * np.array([1, 1, 0.2])
    bg, ba = rng.normal(0, 0.002, 3), rng.normal(0, 0.02, 3)
    T = n_imu * imu_dt
    t = 50.0 + seed
    frames, states, imus, ts = [], [], [None], []
    for k in range(n_frames):
        ns = navstate(P, V, R, bg, ba)
        Rcw, tcw = cam_pose_from_navstate(ns, cam)
        frames.append(base.copy() if k == 0 else render_view(base, cam, Rcw, tcw, seed=seed * 1009 + k))
        states.append(ns); ts.append(t)
        if k == n_frames - 1:
            break
        omega = rng.normal(0, 0.12, 3)
        a_w = rng.normal(0, 0.8, 3) * np.array([1, 1, 0.3]) - 0.8 * V      # keeps the speed bounded
        stamps = t + imu_dt * (np.arange(n_imu) + 0.3)
        imu = np.zeros((n_imu, 7))
        for j, tj in enumerate(stamps):
            Rt = R @ _rotvec_to_R(omega * (tj - t))
            imu[j, :3] = omega + bg + rng.normal(0, 1e-3, 3)
            imu[j, 3:6] = Rt.T @ (a_w - GRAVITY_CAM_WORLD) + ba + rng.normal(0, 1e-2, 3)
            imu[j, 6] = tj
        imus.append(imu)
        P = P + V * T + 0.5 * a_w * T * T
        V = V + a_w * T
        R = R @ _rotvec_to_R(omega * T)
        t = t + T
    return dict(frames=np.stack(frames), ns_true=np.stack(states), imu=imus, t=np.array(ts), cam=cam,
                gw=GRAVITY_CAM_WORLD.copy(), base=base)


def make_periodic_stream(seed, n_frames=8, w=752, h=480, n_imu=10, imu_dt=0.005, nfeat_hint=None, dist=None):
    """A closed-loop mono-inertial stream: poses, velocities and images are periodic with period
    n_frames * n_imu * imu_dt, so a tracker can run over it for any number of steps (frame k of the run is
    frame k % n_frames of the stream; time keeps increasing). IMU samples come from the analytic trajectory.
    Returns dict(frames [n,h,w], ns_true [n,22], pose_true [n,12] (Rcw,tcw double), imu [n,n_imu,7] with
    imu[j] covering frame j-1 -> j (j = 0: frame n-1 -> n == 0) and stamps relative to the period start,
    t [n] frame stamps in [0, T), period T, cam, gw)."""
    rng = np.random.Generator(np.random.PCG64(seed + 987001))
    cam = euroc_cam()
    Rbc, Pbc = cam[4:13].reshape(3, 3), cam[13:16]
    base = make_image(seed, w, h)
    dtf = n_imu * imu_dt
    T = n_frames * dtf
    wp = 2 * np.pi / T
    A = rng.uniform(0.02, 0.05, 3) * np.array([1, 1, 0.4]); phP = rng.uniform(0, 2 * np.pi, 3)
    Th = np.deg2rad(rng.uniform(0.5, 1.5, 3)); phR = rng.uniform(0, 2 * np.pi, 3)
    bg, ba = rng.normal(0, 0.002, 3), rng.normal(0, 0.02, 3)
    R0 = Rbc.T.copy()                                    # camera starts near Tcw = I
    P0 = -R0 @ Pbc

    def traj(t):
        P = P0 + A * np.sin(wp * t + phP)
        V = A * wp * np.cos(wp * t + phP)
        Acc = -A * wp * wp * np.sin(wp * t + phP)
        th = Th * np.sin(wp * t + phR); thd = Th * wp * np.cos(wp * t + phR)
        R = R0 @ _rotvec_to_R(th)
        n = np.linalg.norm(th)
        if n < 1e-9:
            Jr = np.eye(3)
        else:
            k = th / n; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            Jr = np.eye(3) - (1 - np.cos(n)) / n * K + (1 - np.sin(n) / n) * K @ K
        return P, V, Acc, R, Jr @ thd

    frames, states, poses, imus, ts = [], [], [], [], []
    for j in range(n_frames):
        t = j * dtf
        P, V, _, R, _ = traj(t)
        ns = navstate(P, V, R, bg, ba)
        Rcw, tcw = cam_pose_from_navstate(ns, cam)
        frames.append(render_view(base, cam, Rcw, tcw, seed=seed * 1013 + j, dist=dist))
        states.append(ns); poses.append(np.concatenate([Rcw.ravel(), tcw])); ts.append(t)
        # IMU between frame j-1 and j (j = 0 closes the loop: stamps in (T - dtf, T))
        tstart = (j - 1) * dtf if j > 0 else T - dtf
        imu = np.zeros((n_imu, 7))
        for q in range(n_imu):
            tq = tstart + imu_dt * (q + 0.3)
            _, _, Acc, Rq, om = traj(tq)
            imu[q, :3] = om + bg + rng.normal(0, 1e-3, 3)
            imu[q, 3:6] = Rq.T @ (Acc - GRAVITY_CAM_WORLD) + ba + rng.normal(0, 1e-2, 3)
            imu[q, 6] = tq
        imus.append(imu)
    return dict(frames=np.stack(frames), ns_true=np.stack(states), pose_true=np.stack(poses), imu=np.stack(imus), t=np.array(ts),
                period=T, frame_dt=dtf, cam=cam, gw=GRAVITY_CAM_WORLD.copy(), base=base)


def plane_points_f32(kps_xy, pose12_true, cam):
    """numpy twin of viorb_synth_plane_points_device (same FP64 operation order, then float32)."""
    T = np.asarray(pose12_true, np.float64)
    fx, fy, cx, cy = cam[:4]
    dx = (kps_xy[:, 0].astype(np.float64) - cx) / fx
    dy = (kps_xy[:, 1].astype(np.float64) - cy) / fy
    rx = T[0] * dx + T[3] * dy + T[6]; ry = T[1] * dx + T[4] * dy + T[7]; rz = T[2] * dx + T[5] * dy + T[8]
    ox = -(T[0] * T[9] + T[3] * T[10] + T[6] * T[11]); oy = -(T[1] * T[9] + T[4] * T[10] + T[7] * T[11])
    oz = -(T[2] * T[9] + T[5] * T[10] + T[8] * T[11])
    s = (PLANE_Z0 - oz) / rz
    return np.stack([ox + s * rx, oy + s * ry, oz + s * rz], 1).astype(np.float32)


def local_points_f32(octaves, pose12_true, Pw, scale_factors):
    """numpy twin of viorb_synth_local_points_device (same FP64 operation order, one rounding to float32):
    pts_f [n,8] = Pw3 normal3 minDist maxDist of points created from one frame with true pose pose12_true."""
    T = np.asarray(pose12_true, np.float64)
    ox = -(T[0] * T[9] + T[3] * T[10] + T[6] * T[11]); oy = -(T[1] * T[9] + T[4] * T[10] + T[7] * T[11])
    oz = -(T[2] * T[9] + T[5] * T[10] + T[8] * T[11])
    P = np.asarray(Pw, np.float32).astype(np.float64)
    dx, dy, dz = P[:, 0] - ox, P[:, 1] - oy, P[:, 2] - oz
    dist = np.sqrt(dx * dx + dy * dy + dz * dz)
    sf = np.asarray(scale_factors, np.float32).astype(np.float64)
    maxd = dist * sf[np.asarray(octaves)]
    mind = maxd / sf[len(sf) - 1]
    return np.concatenate([np.asarray(Pw, np.float32), np.stack([dx / dist, dy / dist, dz / dist, mind, maxd], 1).astype(np.float32)], 1)


def make_local_map(kps, Pw, ns_ref, cam, scale_factors):
    """Local map points from the keypoints of a reference key frame (MapPoint::UpdateNormalAndDepth, reference
    src/MapPoint.cc:339-378): normal = unit viewing ray, mfMaxDistance = dist * scale[octave],
    mfMinDistance = mfMaxDistance / scale[nLevels-1]. Returns pts_f [n,8] float32 = Pw3 normal3 minDist maxDist."""
    Rcw, tcw = cam_pose_from_navstate(ns_ref, cam)
    Ow = -Rcw.T @ tcw
    PO = Pw.astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    normal = PO / dist[:, None]
    sf = np.asarray(scale_factors, np.float64)
    maxd = dist * sf[kps["octave"]]
    mind = maxd / sf[-1]
    return np.concatenate([Pw.astype(np.float64), normal, mind[:, None], maxd[:, None]], 1).astype(np.float32)


def make_se3_problem(seed, n_points=300, stereo_frac=0.0, outlier_frac=0.05, bf=386.1448, w=752, h=480):
    """A vision-only pose problem (Optimizer::PoseOptimization(Frame*)): points in front of a camera with pose
    (Rcw, tcw), float32 observations, an initial pose a few cm / tenths of a degree off. obs7 = Xw3 u v ur invSigma2."""
    rng = np.random.Generator(np.random.PCG64(seed + 5150))
    fx, fy, cx, cy = EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"]
    Rcw = _rotvec_to_R(rng.normal(0, 0.3, 3)); tcw = rng.normal(0, 0.5, 3)
    uv = np.stack([rng.uniform(20, w - 20, n_points), rng.uniform(20, h - 20, n_points)], 1)
    z = rng.uniform(2, 10, n_points)
    Pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    Xw = (Rcw.T @ (Pc - tcw).T).T
    octave = rng.integers(0, 8, n_points)
    sig = 1.2 ** octave
    inv_s2 = (1.0 / (np.float32(1.2) ** octave).astype(np.float32) ** 2).astype(np.float64)
    o = uv + rng.normal(0, 1, uv.shape) * sig[:, None]
    ur = o[:, 0] - bf / z + rng.normal(0, 1, n_points) * sig
    bad = rng.random(n_points) < outlier_frac
    o[bad] += rng.choice([-1, 1], (bad.sum(), 2)) * rng.uniform(15, 25, (bad.sum(), 2))
    is_stereo = rng.random(n_points) < stereo_frac
    ur = np.where(is_stereo, ur, -1.0)
    obs7 = np.concatenate([np.float32(Xw).astype(np.float64), np.float32(o).astype(np.float64), np.float32(ur).astype(np.float64)[:, None],
                           inv_s2[:, None]], 1)
    R0 = _rotvec_to_R(rng.normal(0, 0.004, 3)) @ Rcw
    t0 = tcw + rng.normal(0, 0.03, 3)
    pose0 = np.concatenate([R0.ravel(), t0]).astype(np.float32)
    return dict(pose0=pose0, pose_true=np.concatenate([Rcw.ravel(), tcw]), obs7=obs7, intr5=np.array([fx, fy, cx, cy, bf]), outlier_true=bad)


KITTI_K = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448)    # reference Examples/Stereo/KITTI00-02.yaml


def make_stereo_pair(seed, w=1241, h=376, fx=718.856, bf=386.1448, zmin=4.0, zmax=40.0):
    """Rectified stereo pair with a smooth known depth field: right(x, y) = left(x + d(x, y), y), d = bf / Z.
    Returns (left, right, disparity_of_right_pixels [h, w])."""
    rng = np.random.Generator(np.random.PCG64(seed + 777))
    left = make_image(seed, w, h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z = zmin + (zmax - zmin) * (0.5 + 0.5 * np.sin(xx / w * 2.1 + rng.uniform(0, 3)) * np.cos(yy / h * 1.3 + rng.uniform(0, 3)))
    d = bf / z
    right = ndimage.map_coordinates(left.astype(np.float32), [yy, xx + d], order=1, mode="reflect")
    right += np.random.Generator(np.random.PCG64(seed + 778)).normal(0, 1.0, right.shape)
    return left, np.clip(np.rint(right), 0, 255).astype(np.uint8), d


def make_local_ba_problem(seed, W=20, n_points=2000, n_fixed_extra=3, outlier_frac=0.05, pix_sigma=2.0, kf_dt=0.15, imu_dt=0.005,
                          w=752, h=480):
    """A LocalBundleAdjustmentNavState problem: W local key frames on a smooth trajectory, the previous
    key frame and a few older covisible key frames fixed, n_points points each seen by 3..8 key frames, pix_sigma-px
    Gaussian noise, outlier_frac gross outliers at ~20 px. Returns flat arrays (layouts of include/viorb.h) + truth."""
    rng = np.random.Generator(np.random.PCG64(seed + 20202))
    cam = euroc_cam()
    fx, fy, cx, cy = cam[:4]; Rbc, Pbc = cam[4:13].reshape(3, 3), cam[13:16]
    nkf = W + 1 + n_fixed_extra                      # chronological: extras, prev, local window
    n_imu = int(round(kf_dt / imu_dt))
    R = Rbc.T.copy(); Pw = -R @ Pbc; V = rng.normal(0, 0.4, 3) * np.array([1, 1, 0.3])
    bg, ba = rng.normal(0, 0.002, 3), rng.normal(0, 0.02, 3)
    states, preints_imu, t = [], [None], 10.0
    from scipy.spatial.transform import Rotation
    for k in range(nkf):
        states.append(navstate(Pw, V, R, bg, ba))
        if k == nkf - 1:
            break
        omega = rng.normal(0, 0.15, 3); a_w = rng.normal(0, 0.6, 3) * np.array([1, 1, 0.3]) - 0.5 * V
        imu = np.zeros((n_imu, 7))
        for j in range(n_imu):
            tj = t + imu_dt * (j + 0.3)
            Rt = R @ _rotvec_to_R(omega * (tj - t))
            imu[j, :3] = omega + bg + rng.normal(0, 1e-3, 3); imu[j, 3:6] = Rt.T @ (a_w - GRAVITY_CAM_WORLD) + ba + rng.normal(0, 1e-2, 3); imu[j, 6] = tj
        preints_imu.append((imu, t, t + kf_dt))
        Pw = Pw + V * kf_dt + 0.5 * a_w * kf_dt ** 2; V = V + a_w * kf_dt; R = R @ _rotvec_to_R(omega * kf_dt); t += kf_dt
    states = np.stack(states)
    # order for the solver: local window first (chronological), then prev, then extras
    chrono_local = list(range(n_fixed_extra + 1, nkf)); prev_c = n_fixed_extra; extra_c = list(range(n_fixed_extra))
    order = chrono_local + [prev_c] + extra_c
    kfs_true = states[order]
    prev_kf = W
    # points: seen from a random local key frame at depth 2..10 m, then observed by every key frame that sees them
    pts, edges_i, edges_o = [], [], []
    poses = [cam_pose_from_navstate(s, cam) for s in kfs_true]
    sf = np.float32(1.2) ** np.arange(8)
    while len(pts) < n_points:
        k0 = int(rng.integers(0, W))
        u0, v0, z = rng.uniform(30, w - 30), rng.uniform(30, h - 30), rng.uniform(2, 10)
        Rcw, tcw = poses[k0]
        X = Rcw.T @ (np.array([(u0 - cx) / fx * z, (v0 - cy) / fy * z, z]) - tcw)
        vis = []
        for k, (Rk, tk) in enumerate(poses):
            Pc = Rk @ X + tk
            if Pc[2] < 0.5: continue
            uu, vv = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
            if 20 < uu < w - 20 and 20 < vv < h - 20: vis.append((k, uu, vv))
        if len(vis) < 3: continue
        nobs = int(min(len(vis), rng.integers(3, 9)))
        sel = sorted(rng.choice(len(vis), nobs, replace=False))
        pid = len(pts); pts.append(X)
        for si in sel:
            k, uu, vv = vis[si]
            octv = int(rng.integers(0, 8)); sg = pix_sigma * float(sf[octv]) / 2.0
            ou, ov = uu + rng.normal(0, sg), vv + rng.normal(0, sg)
            if rng.random() < outlier_frac: ou += rng.choice([-1, 1]) * rng.uniform(15, 25); ov += rng.choice([-1, 1]) * rng.uniform(15, 25)
            edges_i.append((pid, k)); edges_o.append((np.float32(ou), np.float32(ov), 1.0 / float(np.float32(sf[octv]) ** 2)))
    pts = np.array(pts)
    # IMU pre-integrations of the local key frames (predecessor = prev for the first one), with the predecessor's bias
    from . import synth as _self  # noqa: F401
    imu_list = [preints_imu[c] for c in chrono_local]          # interval ending at chrono index c
    # initial estimates
    kfs0 = kfs_true.copy()
    for i in range(W):
        kfs0[i, :3] += rng.normal(0, 0.02, 3); kfs0[i, 3:6] += rng.normal(0, 0.05, 3)
        q = Rotation.from_quat(kfs0[i, 6:10]) * Rotation.from_rotvec(rng.normal(0, 0.005, 3))
        qq = q.as_quat(); kfs0[i, 6:10] = qq if qq[3] >= 0 else -qq
    pts0 = pts + rng.normal(0, 0.05, pts.shape)
    return dict(kfs=kfs0, kfs_true=kfs_true, n_local=W, prev_kf=prev_kf, imu=imu_list, points=np.float32(pts0).astype(np.float64), points_true=pts,
                edge_idx=np.array(edges_i, np.int32), edge_obs=np.array(edges_o, np.float64), gw=GRAVITY_CAM_WORLD.copy(), cam=cam)


def make_vocabulary(seed, k=10, L=6, flip_bits=(96, 64, 40, 24, 14, 8, 5, 3)):
    """A synthetic DBoW2-shaped ORB vocabulary (the reference's ORBvoc.txt is not distributable with the repo): a complete
    k-ary tree of depth L over 256-bit descriptors, each child = its parent with flip_bits[level] random bits flipped
    (root children are uniform random), node ids in breadth-first order shuffled within a level so that child ids are not
    contiguous (as in a k-means-built file), leaves numbered as words in id order with TF-IDF-like weights in (0, 8] and
    about 0.2 % stopped words (weight 0). Flat layout = include/viorb.h `viorb_vocabulary`."""
    rng = np.random.Generator(np.random.PCG64(seed + 777))
    n_level = [k ** l for l in range(L + 1)]
    n_nodes = sum(n_level)
    base = np.cumsum([0] + n_level)
    desc = np.zeros((n_nodes, 32), np.uint8)
    ids = [np.arange(base[l], base[l + 1]) for l in range(L + 1)]
    for l in range(1, L + 1):
        ids[l] = base[l] + rng.permutation(n_level[l])          # node id of the j-th node (in parent-major order) of level l
    child_start = np.zeros(n_nodes + 1, np.int64)
    child_ids = np.zeros(n_nodes - 1, np.int32)
    counts = np.zeros(n_nodes, np.int64)
    for l in range(L):
        counts[ids[l]] = k
    child_start[1:] = np.cumsum(counts)
    for l in range(L):
        par = ids[l]                                            # parents in order j
        ch = ids[l + 1].reshape(n_level[l], k)                  # children of parent j
        pos = child_start[par][:, None] + np.arange(k)[None, :]
        child_ids[pos.ravel()] = ch.ravel()
        if l == 0:
            d = rng.integers(0, 256, (k, 32), dtype=np.uint8)
        else:
            pd = np.repeat(desc[par], k, axis=0)
            nflip = flip_bits[min(l, len(flip_bits) - 1)]
            bits = rng.integers(0, 256, (len(pd), nflip))
            mask = np.zeros((len(pd), 32), np.uint8)
            np.bitwise_xor.at(mask, (np.arange(len(pd))[:, None].repeat(nflip, 1).ravel(), (bits >> 3).ravel()), (1 << (bits & 7)).astype(np.uint8).ravel())
            d = pd ^ mask
        desc[ch.ravel()] = d
    word_id = np.full(n_nodes, -1, np.int32)
    leaves = np.sort(ids[L])
    word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
    weight = np.zeros(n_nodes)
    wl = rng.uniform(0.05, 8.0, len(leaves)); wl[rng.random(len(leaves)) < 0.002] = 0.0
    weight[leaves] = wl
    return dict(k=k, L=L, child_start=child_start.astype(np.int32), child_ids=child_ids, desc=desc, word_id=word_id, weight=weight)


def descriptors_near_words(seed, voc, n, noise_bits=6):
    """n descriptors, each a random vocabulary leaf with noise_bits random bits flipped (so the tree descent is non-trivial
    but features of one scene cluster in a few nodes)."""
    rng = np.random.Generator(np.random.PCG64(seed + 4242))
    leaves = np.nonzero(voc["word_id"] >= 0)[0]
    d = voc["desc"][rng.choice(leaves, n)].copy()
    for _ in range(noise_bits):
        b = rng.integers(0, 256, n)
        d[np.arange(n), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


KP_NP = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])   # == viorb_keypoint / cv::KeyPoint


def make_two_view_problem(seed, n1=900, n2=950, n_common=500, stereo_frac=0.0, w=752, h=480):
    """Two key frames observing a 3-D point cloud, for SearchForTriangulation / Fuse: keypoints (float32 pixel positions with octave
    and angle), descriptors (noisy copies for common points), vocabulary-like node ids (common points share a node), has_point
    flags, the fundamental matrix F12 (x1^T F12 x2 = 0, as ORB-SLAM's ComputeF12), poses and camera centre. numpy only."""
    rng = np.random.Generator(np.random.PCG64(seed + 31337))
    fx, fy, cx, cy = [np.float32(v) for v in (EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"])]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    R1 = _rotvec_to_R(rng.normal(0, 0.05, 3)); t1 = rng.normal(0, 0.05, 3)
    R2 = _rotvec_to_R(rng.normal(0, 0.08, 3)) @ R1; t2 = t1 + np.array([0.35, 0.05, 0.02]) + rng.normal(0, 0.02, 3)
    def project(R, t, X):
        Pc = (R @ X.T).T + t
        return np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1), Pc[:, 2]
    # common 3-D points in front of both cameras
    X = np.stack([rng.uniform(-3, 3, 4 * n_common), rng.uniform(-2, 2, 4 * n_common), rng.uniform(3, 12, 4 * n_common)], 1)
    uv1, z1 = project(R1, t1, X); uv2, z2 = project(R2, t2, X)
    ok = (z1 > 0.5) & (z2 > 0.5) & (uv1[:, 0] > 20) & (uv1[:, 0] < w - 20) & (uv1[:, 1] > 20) & (uv1[:, 1] < h - 20) & \
         (uv2[:, 0] > 20) & (uv2[:, 0] < w - 20) & (uv2[:, 1] > 20) & (uv2[:, 1] < h - 20)
    X, uv1, uv2 = X[ok][:n_common], uv1[ok][:n_common], uv2[ok][:n_common]
    nc = len(X)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    def frame(n, uvc, salt):
        r = np.random.Generator(np.random.PCG64(seed * 13 + salt))
        k = np.zeros(n, KP_NP)
        k["x"][:nc] = uvc[:, 0] + r.normal(0, 0.7, nc); k["y"][:nc] = uvc[:, 1] + r.normal(0, 0.7, nc)
        k["x"][nc:] = r.uniform(20, w - 20, n - nc); k["y"][nc:] = r.uniform(20, h - 20, n - nc)
        k["octave"] = r.integers(0, 8, n); k["angle"] = r.uniform(0, 360, n); k["size"] = 31 * sf[k["octave"]]; k["class_id"] = -1
        return k
    k1 = frame(n1, uv1, 1); k2 = frame(n2, uv2, 2)
    k2["octave"][:nc] = np.clip(k1["octave"][:nc] + rng.integers(-1, 2, nc), 0, 7)
    k2["angle"][:nc] = (k1["angle"][:nc] + rng.choice([8.0, 8.0, 8.0, 200.0], nc) + rng.normal(0, 3, nc)) % 360
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8); d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d2[:nc] = d1[:nc]
    for _ in range(14):
        b = rng.integers(0, 256, nc); d2[np.arange(nc), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    node1 = rng.integers(0, 60, n1).astype(np.int32); node2 = rng.integers(0, 60, n2).astype(np.int32)
    node2[:nc] = node1[:nc]
    node1[rng.random(n1) < 0.02] = -1
    hp1 = (rng.random(n1) < 0.35).astype(np.uint8); hp2 = (rng.random(n2) < 0.35).astype(np.uint8)
    ur1 = np.where(rng.random(n1) < stereo_frac, k1["x"] - 20.0, -1.0).astype(np.float32)
    ur2 = np.where(rng.random(n2) < stereo_frac, k2["x"] - 20.0, -1.0).astype(np.float32)
    p1 = rng.permutation(n1); p2 = rng.permutation(n2)
    inv2 = np.empty(n2, np.int64); inv2[p2] = np.arange(n2)
    truth = np.full(n1, -1, np.int64); truth[:nc] = np.arange(nc)
    truth = np.where(truth >= 0, inv2[np.maximum(truth, 0)], -1)[p1]
    k1, d1, node1, hp1, ur1 = k1[p1], d1[p1], node1[p1], hp1[p1], ur1[p1]
    k2, d2, node2, hp2, ur2 = k2[p2], d2[p2], node2[p2], hp2[p2], ur2[p2]
    # F12 = K^-T [t12]x R12 K^-1 with R12 = R1 R2^T, t12 = -R1 R2^T t2 + t1 (LocalMapping::ComputeF12), float32 like the cv::Mat
    R12 = R1 @ R2.T; t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)).astype(np.float32)
    Cw1 = (-R1.T @ t1).astype(np.float32)
    pose2 = np.concatenate([R2.ravel(), t2]).astype(np.float32); pose1 = np.concatenate([R1.ravel(), t1]).astype(np.float32)
    return dict(k1=k1, d1=d1, node1=node1, hp1=hp1, ur1=ur1, k2=k2, d2=d2, node2=node2, hp2=hp2, ur2=ur2, F12=F12, Cw1=Cw1, pose1=pose1,
                pose2=pose2, intr4=np.array([fx, fy, cx, cy], np.float32), sf=sf, level_sigma2=(sf * sf).astype(np.float32),
                inv_level_sigma2=(np.float32(1) / (sf * sf)).astype(np.float32), truth12=truth, X=X)


def make_two_view_init_problem(seed, kind="general", n1=400, n2=430, n_matches=300, outlier_share=0.1, noise_px=0.5, w=752, h=480):
    """Two monocular frames with putative matches, for the two-view initialiser (Initializer::Initialize): xy1 [n1,2], xy2 [n2,2]
    undistorted key points (float32), matches12 [n1] (index in frame 2 or -1), K4. Camera 1 is the origin, X2 = R21 X1 + t21.
    kind: "general" (depths 4..12, sideways motion), "planar" (every point on one tilted plane), "low_parallax" (rotation, baseline about
    1e-3 of the depth), "forward" (motion along the optical axis). n_matches matches of which outlier_share point to a random key point
    of frame 2; the other key points of both frames are unmatched clutter (so that Normalize over all key points differs from one over
    the matched ones). Ground truth: R21, t21 (unit), scale = |t| before normalisation, depth1 [n1] = depth in camera 1 of a true match
    (nan otherwise), true12 [n1] (1 for a true match). numpy only."""
    rng = np.random.Generator(np.random.PCG64(seed + 424243))
    fx, fy, cx, cy = [float(np.float32(v)) for v in (EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"])]
    motion = dict(general=((0.03, (-0.55, 0.04, 0.03))), planar=((0.04, (-0.5, 0.06, 0.05))), low_parallax=((0.05, (-0.008, 0.001, 0.0))),
                  forward=((0.02, (0.03, 0.02, -0.7))))[kind]
    R = _rotvec_to_R(rng.normal(0, motion[0], 3)); t = np.array(motion[1]) + rng.normal(0, 0.02, 3) * np.linalg.norm(motion[1])
    m = 6 * n_matches + 64
    uv1 = np.stack([rng.uniform(15, w - 15, m), rng.uniform(15, h - 15, m)], 1)
    ray = np.stack([(uv1[:, 0] - cx) / fx, (uv1[:, 1] - cy) / fy, np.ones(m)], 1)
    if kind == "planar":
        nrm = np.array([0.3, 0.2, 1.0]); z = 6.0 / (ray @ nrm)            # the plane 0.3 x + 0.2 y + z = 6
    else:
        z = rng.uniform(4.0, 12.0, m)
    X = ray * z[:, None]
    X2 = X @ R.T + t
    uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    ok = (z > 0.5) & (X2[:, 2] > 0.5) & (uv2[:, 0] > 15) & (uv2[:, 0] < w - 15) & (uv2[:, 1] > 15) & (uv2[:, 1] < h - 15)
    uv1, uv2, z = uv1[ok][:n_matches], uv2[ok][:n_matches], z[ok][:n_matches]
    nm = len(uv1)
    assert nm == n_matches and n1 >= nm and n2 >= nm, "not enough visible points / key points for n_matches"
    xy1 = np.concatenate([uv1 + rng.normal(0, noise_px, (nm, 2)), np.stack([rng.uniform(15, w - 15, n1 - nm), rng.uniform(15, h - 15, n1 - nm)], 1)])
    xy2 = np.concatenate([uv2 + rng.normal(0, noise_px, (nm, 2)), np.stack([rng.uniform(15, w - 15, n2 - nm), rng.uniform(15, h - 15, n2 - nm)], 1)])
    match = np.full(n1, -1, np.int64); match[:nm] = np.arange(nm)
    true12 = np.zeros(n1, np.uint8); true12[:nm] = 1
    out = rng.permutation(nm)[:int(round(outlier_share * nm))]
    match[out] = rng.integers(0, n2, len(out)); true12[out] = 0
    depth = np.full(n1, np.nan); depth[:nm] = z; depth[out] = np.nan
    p1, p2 = rng.permutation(n1), rng.permutation(n2)
    inv2 = np.empty(n2, np.int64); inv2[p2] = np.arange(n2)
    match = np.where(match >= 0, inv2[np.maximum(match, 0)], -1)[p1]
    return dict(xy1=xy1[p1].astype(np.float32), xy2=xy2[p2].astype(np.float32), matches12=match.astype(np.int32),
                K4=np.array([fx, fy, cx, cy], np.float32), R21=R, t21=t / np.linalg.norm(t), scale=float(np.linalg.norm(t)), depth1=depth[p1],
                true12=true12[p1], kind=kind)


def make_local_ba_se3_problem(seed, W=8, n_fixed=3, n_points=600, stereo_frac=0.5, outlier_frac=0.05, pix_sigma=1.5, w=1241, h=376):
    """A vision-only LocalBundleAdjustment problem (KITTI-shaped camera): W free key frames + n_fixed fixed ones on a forward-moving
    trajectory, points seen by 3..7 key frames, a mix of mono and stereo observations, Gaussian pixel noise and gross outliers.
    Returns flat arrays (kfs [NK,7] = qx qy qz qw tx ty tz of Tcw, free first) + truth."""
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(seed + 9090))
    fx = fy = 718.856; cx, cy, bf = 607.1928, 185.2157, 386.1448
    nk = W + n_fixed
    poses = []
    p = np.zeros(3); yaw = 0.0
    for k in range(nk):
        Rwc = Rotation.from_euler("y", yaw).as_matrix() @ _rotvec_to_R(rng.normal(0, 0.01, 3))
        poses.append((Rwc.T, -Rwc.T @ p))                                     # Tcw
        p = p + Rwc @ np.array([rng.normal(0, 0.05), rng.normal(0, 0.02), 0.8 + rng.normal(0, 0.1)]); yaw += rng.normal(0, 0.03)
    order = list(range(n_fixed, nk)) + list(range(n_fixed))                   # free (recent) key frames first, then the fixed (older) ones
    poses = [poses[i] for i in order]
    pts, ei, eo = [], [], []
    sf = np.float32(1.2) ** np.arange(8)
    while len(pts) < n_points:
        k0 = int(rng.integers(0, nk)); Rk, tk = poses[k0]
        z = rng.uniform(4, 40); Xc = np.array([(rng.uniform(20, w - 20) - cx) / fx * z, (rng.uniform(20, h - 20) - cy) / fy * z, z])
        X = Rk.T @ (Xc - tk)
        vis = []
        for k, (R, t) in enumerate(poses):
            Pc = R @ X + t
            if Pc[2] < 1.0: continue
            u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
            if 10 < u < w - 10 and 10 < v < h - 10: vis.append((k, u, v, Pc[2]))
        if len(vis) < 3: continue
        sel = sorted(rng.choice(len(vis), int(min(len(vis), rng.integers(3, 8))), replace=False))
        pid = len(pts); pts.append(X)
        for si in sel:
            k, u, v, zc = vis[si]
            octv = int(rng.integers(0, 8)); sg = pix_sigma * float(sf[octv]) / 1.5
            ou, ov = u + rng.normal(0, sg), v + rng.normal(0, sg)
            stereo = rng.random() < stereo_frac and zc < 35
            our = (u - bf / zc + rng.normal(0, sg)) if stereo else -1.0
            if rng.random() < outlier_frac: ou += rng.choice([-1, 1]) * rng.uniform(12, 25)
            ei.append((pid, k)); eo.append((np.float32(ou), np.float32(ov), np.float32(our) if stereo else -1.0, 1.0 / float(np.float32(sf[octv]) ** 2)))
    pts = np.array(pts)
    def to7(R, t):
        q = Rotation.from_matrix(R).as_quat(); q = q if q[3] >= 0 else -q
        return np.concatenate([q, t])
    kfs_true = np.stack([to7(R, t) for R, t in poses])
    kfs = kfs_true.copy()
    for i in range(W):                                                        # perturb the free key frames
        R, t = poses[i]
        Rp = _rotvec_to_R(rng.normal(0, 0.01, 3)) @ R
        kfs[i] = to7(Rp, t + rng.normal(0, 0.05, 3))
    points0 = pts + rng.normal(0, 0.1, pts.shape)
    return dict(kfs=kfs, kfs_true=kfs_true, n_local=W, points=points0, points_true=pts, edge_idx=np.array(ei, np.int32), edge_obs=np.array(eo, np.float64),
                intr5=np.array([fx, fy, cx, cy, bf]))


def make_mapping_problem(seed, J=20, n1=1000, n2=1000, stereo_frac=0.0, w=752, h=480):
    """One current key frame and J neighbour key frames over a common cloud, for map-point creation (LocalMapping::CreateNewMapPoints,
    MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth). Built so that every statement of the per-pair loop is taken:
    baselines from far too short (the baseline test skips the neighbour) to wide, a far shell of points beyond the 0.9998 parallax
    limit, sideways-looking neighbours and wrong partners that triangulate behind a camera, a share of key points with pixel noise
    far above the reprojection gates, octave pairs that violate scale consistency, and `stereo_frac` of the key points with uRight /
    depth so that both UnprojectStereo branches and the 7.8 gates run. Besides what SearchForTriangulation needs (descriptors,
    vocabulary nodes, F12) every neighbour carries `match_gen`, a match12 written here from the truth (true partners, near misses a
    few pixels off, wrong partners): the search's epipolar gate would remove most bad pairs before the vetting sees them.
    Returns dict(cam, kf1, neigh[J], bounds, X). numpy only."""
    rng = np.random.Generator(np.random.PCG64(seed + 424243))
    f32 = np.float32
    fx, fy, cx, cy = [f32(v) for v in (EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"])]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    Kinv = np.linalg.inv(K)
    mb = f32(0.11); mbf = f32(fx * mb)
    sf = (f32(1.2) ** np.arange(8)).astype(np.float32)
    cam = dict(intr4=np.array([fx, fy, cx, cy], np.float32), mb=mb, mbf=mbf, scale_factor=f32(1.2), sf=sf, level_sigma2=(sf * sf).astype(np.float32),
               inv_level_sigma2=(f32(1) / (sf * sf)).astype(np.float32))
    n_near = int(n1 * 0.8)
    dirs = np.stack([rng.uniform(-0.9, 0.9, n1), rng.uniform(-0.55, 0.55, n1), np.ones(n1)], 1)
    depth = np.concatenate([rng.uniform(2.0, 14.0, n_near), rng.uniform(60.0, 900.0, n1 - n_near)])
    R1 = _rotvec_to_R(rng.normal(0, 0.03, 3)); t1 = rng.normal(0, 0.05, 3)
    X = (R1.T @ (dirs * depth[:, None] - t1).T).T                       # cloud: every point is seen by the current key frame
    base_desc = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    base_node = rng.integers(0, 80, n1).astype(np.int32)
    base_oct = rng.integers(0, 8, n1)
    base_angle = rng.uniform(0, 360, n1)

    def project(R, t, P):
        Pc = (R @ P.T).T + t
        z = np.where(np.abs(Pc[:, 2]) < 1e-9, 1e-9, Pc[:, 2])
        return np.stack([fx * Pc[:, 0] / z + cx, fy * Pc[:, 1] / z + cy], 1), Pc[:, 2]

    def frame(R, t, n, salt, is_cur):
        r = np.random.Generator(np.random.PCG64(seed * 977 + salt))
        uv, z = project(R, t, X)
        vis = np.nonzero((z > 0.3) & (uv[:, 0] > 16) & (uv[:, 0] < w - 16) & (uv[:, 1] > 16) & (uv[:, 1] < h - 16))[0]
        if not is_cur:
            vis = vis[r.random(len(vis)) < 0.85][:n - n // 8]
        nv = len(vis)
        n_dup = 0 if is_cur else min(n - nv, nv // 8)                        # near misses: a second feature a few pixels off the true one
        k = np.zeros(n, KP_NP); pid = np.full(n, -1, np.int64)
        sig = np.where(r.random(nv) < 0.12, 6.0, 0.6)                        # a share far above the chi2 gates
        octv = base_oct[vis] if is_cur else np.clip(base_oct[vis] + r.integers(-1, 2, nv), 0, 7)
        if not is_cur:
            bad = r.random(nv) < 0.08
            octv = np.where(bad, (base_oct[vis] + 4) % 8, octv)              # violates scale consistency
        k["x"][:nv] = uv[vis, 0] + r.normal(0, 1, nv) * sig; k["y"][:nv] = uv[vis, 1] + r.normal(0, 1, nv) * sig
        k["octave"][:nv] = octv; pid[:nv] = vis
        dup = r.choice(nv, n_dup, replace=False) if n_dup else np.zeros(0, np.int64)
        ang = r.uniform(0, 2 * np.pi, n_dup); rad = r.uniform(2.5, 9.0, n_dup)
        k["x"][nv:nv + n_dup] = k["x"][dup] + rad * np.cos(ang); k["y"][nv:nv + n_dup] = k["y"][dup] + rad * np.sin(ang)
        k["octave"][nv:nv + n_dup] = k["octave"][dup]
        near = np.full(n, -1, np.int64); near[nv:nv + n_dup] = vis[dup] if n_dup else 0
        m = nv + n_dup
        k["x"][m:] = r.uniform(16, w - 16, n - m); k["y"][m:] = r.uniform(16, h - 16, n - m); k["octave"][m:] = r.integers(0, 8, n - m)
        k["angle"] = r.uniform(0, 360, n); k["angle"][:nv] = (base_angle[vis] + r.normal(0, 3, nv)) % 360
        k["size"] = 31 * sf[k["octave"]]; k["class_id"] = -1
        d = r.integers(0, 256, (n, 32), dtype=np.uint8); d[:nv] = base_desc[vis]; d[nv:m] = base_desc[vis[dup]] if n_dup else d[nv:m]
        for _ in range(9):
            bsel = r.integers(0, 256, m); d[np.arange(m), bsel >> 3] ^= (1 << (bsel & 7)).astype(np.uint8)
        node = r.integers(0, 80, n).astype(np.int32); node[:nv] = base_node[vis]
        if n_dup:
            node[nv:m] = base_node[vis[dup]]
        node[r.random(n) < 0.02] = -1
        zt = np.full(n, -1.0); zt[:nv] = z[vis]
        if n_dup:
            zt[nv:m] = z[vis[dup]]
        stereo = (r.random(n) < stereo_frac) & (zt > 0) & (zt < 40.0)
        zn = zt * (1 + r.normal(0, 0.01, n))
        ur = np.where(stereo, k["x"] - mbf / np.where(stereo, zn, 1.0) + r.normal(0, 0.4, n), -1.0).astype(np.float32)
        dep = np.where(stereo, zn, -1.0).astype(np.float32)
        hp = (r.random(n) < 0.3).astype(np.uint8)
        # the distorted key points KeyFrame::UnprojectStereo reads: a mild radial shift of the undistorted ones
        dx, dy = (k["x"] - cx) / fx, (k["y"] - cy) / fy
        rr = dx * dx + dy * dy
        xy_dist = np.stack([cx + fx * dx * (1 - 0.02 * rr), cy + fy * dy * (1 - 0.02 * rr)], 1).astype(np.float32)
        perm = r.permutation(n)
        Ow = (-R.T @ t).astype(np.float32)
        return dict(kps=k[perm], desc=d[perm], node=node[perm], hp=hp[perm], ur=ur[perm], depth=dep[perm], xy_dist=np.ascontiguousarray(xy_dist[perm]),
                    pid=pid[perm], near=near[perm], pose12=np.concatenate([R.ravel(), t]).astype(np.float32), Ow=Ow, R=R, t=t)

    kf1 = frame(R1, t1, n1, 1, True)
    of_pid1 = np.full(n1, -1, np.int64); of_pid1[kf1["pid"][kf1["pid"] >= 0]] = np.nonzero(kf1["pid"] >= 0)[0]
    C1 = -R1.T @ t1
    baselines = np.concatenate([[0.004, 0.03], np.geomspace(0.08, 1.6, max(J - 2, 1))])[:J]
    neigh = []
    for j in range(J):
        dirn = rng.normal(0, 1, 3) * np.array([1.0, 0.4, 0.6]); dirn /= np.linalg.norm(dirn)
        yaw = rng.normal(0, 0.06, 3)
        if j % 5 == 4:
            yaw = yaw + np.array([0.0, rng.choice([-1.0, 1.0]) * 0.45, 0.0])  # looks sideways: wrong partners triangulate behind a camera
        R2 = _rotvec_to_R(yaw) @ R1
        C2 = C1 + baselines[j] * dirn
        t2 = -R2 @ C2
        kf = frame(R2, t2, n2, 100 + j, False)
        R12 = R1 @ R2.T; t12 = -R12 @ t2 + t1
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        kf["F12"] = (Kinv.T @ tx @ R12 @ Kinv).astype(np.float32)
        _, z2 = project(R2, t2, X[:n_near])
        kf["median_depth"] = f32(np.median(z2[z2 > 0]))
        kf["kf2_first"] = np.uint8(rng.integers(0, 2))
        # match12 from the truth: true partners, near misses, wrong partners, and unmatched
        of_pid2 = np.full(n1, -1, np.int64); sel = kf["pid"] >= 0; of_pid2[kf["pid"][sel]] = np.nonzero(sel)[0]
        near_of = np.full(n1, -1, np.int64); sel = kf["near"] >= 0; near_of[kf["near"][sel]] = np.nonzero(sel)[0]
        mg = np.full(n1, -1, np.int32)
        for i1 in range(n1):
            p = kf1["pid"][i1]
            u = rng.random()
            if p >= 0 and of_pid2[p] >= 0 and u < 0.8:
                mg[i1] = near_of[p] if (near_of[p] >= 0 and u < 0.25) else of_pid2[p]
            elif u > 0.88:
                mg[i1] = rng.integers(0, n2)
        kf["match_gen"] = mg
        neigh.append(kf)
    return dict(cam=cam, kf1=kf1, neigh=neigh, bounds=np.array([0, w, 0, h], np.float32), X=X)


def make_vi_init_problem(seed, N, kf_dt=0.25, imu_dt=0.005, scale=3.7, noise=0.0, G=9.8012, Tbc=None):
    """A stream for the visual-inertial initialisation (LocalMapping::TryInitVIO) with its truth: N key frames kf_dt apart on a smooth
    body trajectory with translational and rotational excitation; IMU samples every imu_dt with the true biases added (and, with
    noise > 0, white noise of noise * 0.01 rad/s and noise * 0.1 m/s^2 per sample); key-frame camera poses Twb Tbc with positions
    divided by `scale`; the world frame rotated so that gravity is a general vector. Tbc: use this camera-body transform instead of the
    seed's own (streams of one batch share a configuration).
    Returns dict(twc12 [N,12] f32 = Rwc(9) twc(3), kf_time [N], imu [total,7], imu_start [N+1] (interval i = samples between key frames
    i - 1 and i), Tbc [4,4], g, truth = dict(s, gw, bg, ba, kf_vel [N,3] = body velocity in the world frame at the key frames))."""
    r = np.random.default_rng(seed)
    amp, fr, ph = r.uniform(0.3, 1.0, 3), r.uniform(0.2, 0.8, 3), r.uniform(0, 6.28, 3)
    ramp, rfr, rph = r.uniform(0.1, 0.4, 3), r.uniform(0.2, 0.7, 3), r.uniform(0, 6.28, 3)
    pos = lambda t: amp * np.sin(2 * np.pi * fr * t + ph)
    acc = lambda t: -amp * (2 * np.pi * fr) ** 2 * np.sin(2 * np.pi * fr * t + ph)
    Rw0 = _rotvec_to_R(r.normal(size=3))                      # visual world against the inertial frame
    gw = Rw0 @ np.array([0, 0, G])
    Rot = lambda t: Rw0 @ _rotvec_to_R(ramp * np.sin(2 * np.pi * rfr * t + rph))
    bg, ba = r.normal(size=3) * 0.02, r.normal(size=3) * 0.1
    own = np.eye(4)
    own[:3, :3] = _rotvec_to_R(r.normal(size=3) * 0.5 + np.array([0, 0, 1.57])); own[:3, 3] = r.normal(size=3) * 0.05
    Tbc = own if Tbc is None else np.asarray(Tbc, np.float64).reshape(4, 4)
    n_imu = int(round(kf_dt / imu_dt))
    tk = np.arange(N) * kf_dt
    twc12 = np.zeros((N, 12), np.float32)
    chunks, start = [], np.zeros(N + 1, np.int32)
    for i in range(N):
        Twb = np.eye(4); Twb[:3, :3] = Rot(tk[i]); Twb[:3, 3] = Rw0 @ pos(tk[i])
        T = Twb @ Tbc
        twc12[i, :9] = T[:3, :3].ravel(); twc12[i, 9:] = T[:3, 3] / scale
        if i > 0:
            S = np.zeros((n_imu, 7))
            for k in range(n_imu):
                t0 = tk[i - 1] + k * imu_dt
                tm = t0 + imu_dt / 2
                dR = Rot(t0).T @ Rot(t0 + imu_dt)             # the constant rate that carries R(t0) to R(t0 + imu_dt)
                th = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
                w = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / (2 * np.sin(th)) * th / imu_dt if th > 1e-12 else np.zeros(3)
                a = Rot(tm).T @ (Rw0 @ acc(tm) - gw)
                S[k, :3] = w + bg + r.normal(size=3) * noise * 0.01
                S[k, 3:6] = a + ba + r.normal(size=3) * noise * 0.1
                S[k, 6] = t0
            chunks.append(S)
        start[i + 1] = start[i] + (n_imu if i > 0 else 0)
    imu = np.concatenate(chunks) if chunks else np.zeros((0, 7))
    kf_vel = np.stack([Rw0 @ (amp * 2 * np.pi * fr * np.cos(2 * np.pi * fr * t + ph)) for t in tk])
    return dict(twc12=twc12, kf_time=tk, imu=imu, imu_start=start, Tbc=Tbc, g=G, truth=dict(s=scale, gw=gw, bg=bg, ba=ba, kf_vel=kf_vel))


def make_global_ba_problem(seed, N=21, n_points=None, revisit_frac=0.0, n_fixed=1, pix_sigma=2.0, kf_dt=0.15, imu_dt=0.005, w=752, h=480,
                           preint_fn=None):
    """A GlobalBundleAdjustmentNavState problem: N chronological key frames on a smooth trajectory past a point cloud (the first n_fixed
    fixed, prev[i] = i - 1), n_points points (default 40 per key frame) each seen by a contiguous run of 3..12 key frames; a revisit_frac
    share of them is seen again by a distant run, so that the reduced matrix is not banded. Pre-integrations: preint_fn(stream, bg, ba)
    -> [N,142], default viorb_preintegrate_intervals (needs a device). Initial states are perturbed as make_local_ba_problem perturbs
    them. Returns flat arrays in the layouts of include/viorb.h + the truth + the IMU stream (kf_time, imu, imu_start)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(seed + 70707))
    n_points = 40 * N if n_points is None else n_points
    cam = euroc_cam()
    fx, fy, cx, cy = cam[:4]; Rbc, Pbc = cam[4:13].reshape(3, 3), cam[13:16]
    n_imu = int(round(kf_dt / imu_dt))
    R = Rbc.T.copy(); Pw = -R @ Pbc; V = rng.normal(0, 0.4, 3) * np.array([1, 1, 0.3])
    bg, ba = rng.normal(0, 0.002, 3), rng.normal(0, 0.02, 3)
    states, chunks, start, t = [], [], np.zeros(N + 1, np.int32), 10.0
    kf_time = 10.0 + kf_dt * np.arange(N)
    for k in range(N):
        states.append(navstate(Pw, V, R, bg, ba))
        start[k + 1] = start[k] + (n_imu if k > 0 else 0)
        if k == N - 1:
            break
        omega = rng.normal(0, 0.15, 3); a_w = rng.normal(0, 0.6, 3) * np.array([1, 1, 0.3]) - 0.5 * V
        imu = np.zeros((n_imu, 7))
        for j in range(n_imu):
            tj = t + imu_dt * (j + 0.3)
            Rt = R @ _rotvec_to_R(omega * (tj - t))
            imu[j, :3] = omega + bg + rng.normal(0, 1e-3, 3); imu[j, 3:6] = Rt.T @ (a_w - GRAVITY_CAM_WORLD) + ba + rng.normal(0, 1e-2, 3); imu[j, 6] = tj
        chunks.append(imu)
        Pw = Pw + V * kf_dt + 0.5 * a_w * kf_dt ** 2; V = V + a_w * kf_dt; R = R @ _rotvec_to_R(omega * kf_dt); t += kf_dt
    kfs_true = np.stack(states)
    stream = dict(kf_time=kf_time, imu=np.concatenate(chunks) if chunks else np.zeros((0, 7)), imu_start=start)
    if preint_fn is None:
        from .vi_init import PreintegrateIntervals
        preint_fn = lambda s, g, a: PreintegrateIntervals(s, g, a, clamp=False)
    preint = np.ascontiguousarray(preint_fn(stream, bg, ba), np.float64).reshape(N, 142)
    poses = [cam_pose_from_navstate(s, cam) for s in kfs_true]
    sf = np.float32(1.2) ** np.arange(8)
    pts, edges_i, edges_o = [], [], []

    def observe(pid, X, ks):
        n = 0
        for k in ks:
            Pc = poses[k][0] @ X + poses[k][1]
            if Pc[2] < 0.5: continue
            uu, vv = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
            if not (-w < uu < 2 * w and -h < vv < 2 * h): continue
            octv = int(rng.integers(0, 8)); sg = pix_sigma * float(sf[octv]) / 2.0
            edges_i.append((pid, k)); edges_o.append((np.float32(uu + rng.normal(0, sg)), np.float32(vv + rng.normal(0, sg)), 1.0 / float(np.float32(sf[octv]) ** 2)))
            n += 1
        return n
    while len(pts) < n_points:
        run = int(min(N, rng.integers(3, 13))); k0 = int(rng.integers(0, N - run + 1))
        kc = k0 + run // 2
        u0, v0, z = rng.uniform(30, w - 30), rng.uniform(30, h - 30), rng.uniform(2, 10)
        Rcw, tcw = poses[kc]
        X = Rcw.T @ (np.array([(u0 - cx) / fx * z, (v0 - cy) / fy * z, z]) - tcw)
        pid = len(pts)
        m0 = len(edges_i)
        ks = list(range(k0, k0 + run))
        if rng.random() < revisit_frac and N > 2 * run + 8:
            run2 = int(rng.integers(3, 13)); far = [k for k in range(0, N - run2 + 1) if k + run2 <= k0 - 8 or k >= k0 + run + 8]
            if far:
                k2 = int(far[int(rng.integers(0, len(far)))]); ks = sorted(ks + list(range(k2, k2 + run2)))
        if observe(pid, X, ks) < 2:
            del edges_i[m0:], edges_o[m0:]
            continue
        pts.append(X)
    pts = np.array(pts).reshape(-1, 3)
    kfs0 = kfs_true.copy()
    for i in range(n_fixed, N):
        kfs0[i, :3] += rng.normal(0, 0.02, 3); kfs0[i, 3:6] += rng.normal(0, 0.05, 3)
        q = Rotation.from_quat(kfs0[i, 6:10]) * Rotation.from_rotvec(rng.normal(0, 0.005, 3))
        qq = q.as_quat(); kfs0[i, 6:10] = qq if qq[3] >= 0 else -qq
    pts0 = pts + rng.normal(0, 0.05, pts.shape)
    prev = np.arange(-1, N - 1, dtype=np.int32); fixed = np.zeros(N, np.uint8); fixed[:n_fixed] = 1
    return dict(kfs=kfs0, kfs_true=kfs_true, prev=prev, fixed=fixed, preint=preint, points=np.float32(pts0).astype(np.float64), points_true=pts,
                edge_idx=np.array(edges_i, np.int32).reshape(-1, 2), edge_obs=np.array(edges_o, np.float64).reshape(-1, 3),
                gw=GRAVITY_CAM_WORLD.copy(), cam=cam, stream=stream, bias=(bg, ba))


def make_global_ba_se3_problem(seed, N=12, stereo_frac=0.5, revisit_frac=0.0, n_fixed=1, n_points=None, outlier_frac=0.03, pix_sigma=1.5,
                               step=0.3, w=1241, h=376):
    """A vision-only Optimizer::BundleAdjustment problem (KITTI-shaped camera, as make_local_ba_se3_problem): N chronological key frames
    creeping forward (`step` metres apart, so that a point stays in front of many of them), the first n_fixed fixed; n_points points
    (default 30 per key frame), each seen by a contiguous run of 3..7 key frames (about 5); a revisit_frac share of them is seen again by
    a distant run (loop re-observations, kept where the point still projects in front of the camera), so that the reduced matrix is not
    banded. stereo_frac of the observations closer than 35 m carry uRight; outlier_frac of them are gross outliers. The start values
    (perturbed poses, noisy points) are rounded through float, as a map holds them. Returns flat arrays in the layouts of
    include/viorb.h (kfs [N,7] = qx qy qz qw tx ty tz of Tcw, edge_obs [E,4] = u v uRight invSigma2, intr5) + the truth. numpy / scipy only."""
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(seed + 515151))
    fx = fy = 718.856; cx, cy, bf = 607.1928, 185.2157, 386.1448
    n_points = 30 * N if n_points is None else n_points
    poses, p, yaw = [], np.zeros(3), 0.0
    for k in range(N):
        Rwc = Rotation.from_euler("y", yaw).as_matrix() @ _rotvec_to_R(rng.normal(0, 0.01, 3))
        poses.append((Rwc.T, -Rwc.T @ p))                                     # Tcw
        p = p + Rwc @ np.array([rng.normal(0, 0.03), rng.normal(0, 0.02), step + rng.normal(0, 0.03)]); yaw += rng.normal(0, 0.01)
    sf = np.float32(1.2) ** np.arange(8)
    pts, ei, eo = [], [], []

    def observe(pid, X, ks):
        n = 0
        for k in ks:
            Pc = poses[k][0] @ X + poses[k][1]
            if Pc[2] < 1.0: continue
            u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
            if not (-0.5 * w < u < 1.5 * w and -0.5 * h < v < 1.5 * h): continue
            octv = int(rng.integers(0, 8)); sg = pix_sigma * float(sf[octv]) / 1.5
            ou, ov = u + rng.normal(0, sg), v + rng.normal(0, sg)
            stereo = rng.random() < stereo_frac and Pc[2] < 35 and u - bf / Pc[2] > 30      # uRight stays positive under the noise
            our = (u - bf / Pc[2] + rng.normal(0, sg)) if stereo else -1.0
            if rng.random() < outlier_frac: ou += rng.choice([-1, 1]) * rng.uniform(12, 25)
            ei.append((pid, k)); eo.append((np.float32(ou), np.float32(ov), np.float32(our) if stereo else -1.0, 1.0 / float(np.float32(sf[octv]) ** 2)))
            n += 1
        return n
    while len(pts) < n_points:
        run = int(min(N, rng.integers(3, 8))); k0 = int(rng.integers(0, N - run + 1))
        Rcw, tcw = poses[k0 + run // 2]
        z = rng.uniform(6, 40)
        X = Rcw.T @ (np.array([(rng.uniform(20, w - 20) - cx) / fx * z, (rng.uniform(20, h - 20) - cy) / fy * z, z]) - tcw)
        ks = list(range(k0, k0 + run))
        if rng.random() < revisit_frac and N > 2 * run + 8:
            run2 = int(rng.integers(3, 8)); far = [k for k in range(0, N - run2 + 1) if k + run2 <= k0 - 8 or k >= k0 + run + 8]
            if far:
                k2 = int(far[int(rng.integers(0, len(far)))]); ks = sorted(ks + list(range(k2, k2 + run2)))
        m0 = len(ei)
        if observe(len(pts), X, ks) < 2:
            del ei[m0:], eo[m0:]
            continue
        pts.append(X)
    pts = np.array(pts).reshape(-1, 3)

    def to7(R, t):
        q = Rotation.from_matrix(R).as_quat(); q = q if q[3] >= 0 else -q
        return np.concatenate([q, t])
    kfs_true = np.stack([to7(R, t) for R, t in poses])
    kfs = kfs_true.copy()
    for i in range(N):
        R, t = poses[i]
        if i >= n_fixed:
            R, t = _rotvec_to_R(rng.normal(0, 0.01, 3)) @ R, t + rng.normal(0, 0.05, 3)
        kfs[i] = to7(np.float32(R).astype(np.float64), np.float32(t).astype(np.float64))     # KeyFrame::Tcw is a float matrix
    fixed = np.zeros(N, np.uint8); fixed[:n_fixed] = 1
    return dict(kfs=kfs, kfs_true=kfs_true, fixed=fixed, points=np.float32(pts + rng.normal(0, 0.1, pts.shape)).astype(np.float64), points_true=pts,
                edge_idx=np.array(ei, np.int32).reshape(-1, 2), edge_obs=np.array(eo, np.float64).reshape(-1, 4), intr5=np.array([fx, fy, cx, cy, bf]))


def _l1_normalised(words, weights):
    """Ascending unique words and their summed weights divided by the norm, the norm summed in ascending word order (BowVector::normalize)."""
    acc = {}
    for w, v in zip(words.tolist(), weights.tolist()):
        acc[w] = acc.get(w, 0.0) + v
    ids = sorted(acc)
    norm = 0.0
    for k in ids:
        norm += acc[k]
    return np.array(ids, np.int32), np.array([acc[k] / norm for k in ids], np.float64)


def _place_words(rng, N, per_kf, n_words, place_len, pool_frac, revisit_at):
    """The word draws of a key-frame sequence that revisits its start: key frame i looks at place i // place_len, from revisit_at * N on at
    the places of the start again; pool_frac of its words come from the place's pool of 2 * per_kf words, the rest from anywhere."""
    first_revisit = int(revisit_at * N)
    n_places = (N + place_len - 1) // place_len
    pools = [rng.choice(n_words, min(2 * per_kf, n_words), replace=False) for _ in range(n_places)]
    out = []
    for i in range(N):
        place = (i if i < first_revisit else i - first_revisit) // place_len
        n_pool = int(pool_frac * per_kf)
        out.append(np.concatenate([rng.choice(pools[place], n_pool), rng.integers(0, n_words, per_kf - n_pool)]))
    return out


def _place_graph(rng, N, erase_frac, n_connected):
    """The database side of a place problem: key frames 0 .. N - 2 are the slots, key frame N - 1 asks. The last n_connected slots are
    connected to it, erase_frac of the others are erased, and a slot's covisibles are its ten nearest slots, nearest first."""
    S = N - 1
    connected = list(range(max(S - n_connected, 0), S))
    free = [s for s in range(S) if s not in connected]
    erased = sorted(rng.choice(free, int(erase_frac * S), replace=False).tolist()) if free and erase_frac > 0 else []
    covis10 = np.full((S, 10), -1, np.int32)
    for s in range(S):
        near = [t for d in range(1, 11) for t in (s - d, s + d) if 0 <= t < S][:10]
        covis10[s, :len(near)] = near
    return connected, erased, covis10


def make_place_problem(seed, N=48, per_kf=120, n_words=4096, place_len=12, pool_frac=0.7, revisit_at=0.75, erase_frac=0.1, n_connected=6):
    """A place-recognition problem built as BoW vectors directly: dict(n_words, bows = N (ids, vals) pairs — the first N - 1 are the
    database's slots in add order, the last one is the query —, connected, erased, covis10 [N - 1, 10])."""
    rng = np.random.Generator(np.random.PCG64(seed + 9090))
    idf = rng.uniform(0.05, 8.0, n_words)
    bows = [_l1_normalised(w, idf[w]) for w in _place_words(rng, N, per_kf, n_words, place_len, pool_frac, revisit_at)]
    connected, erased, covis10 = _place_graph(rng, N, erase_frac, n_connected)
    return dict(n_words=n_words, bows=bows, connected=connected, erased=erased, covis10=covis10)


def make_place_descriptors(seed, voc, N=24, per_kf=100, noise_bits=2, place_len=6, pool_frac=0.7, revisit_at=0.75, erase_frac=0.1, n_connected=3):
    """The same construction through a vocabulary (make_vocabulary): dict(desc = N arrays [per_kf, 32] near the drawn words' leaves,
    connected, erased, covis10); the BoW vectors come out of the transform."""
    rng = np.random.Generator(np.random.PCG64(seed + 9191))
    leaf_of_word = np.nonzero(voc["word_id"] >= 0)[0]
    leaf_of_word = leaf_of_word[np.argsort(voc["word_id"][leaf_of_word])]
    desc = []
    for w in _place_words(rng, N, per_kf, len(leaf_of_word), place_len, pool_frac, revisit_at):
        d = voc["desc"][leaf_of_word[w]].copy()
        for _ in range(noise_bits):
            b = rng.integers(0, 256, len(d))
            d[np.arange(len(d)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
        desc.append(d)
    connected, erased, covis10 = _place_graph(rng, N, erase_frac, n_connected)
    return dict(desc=desc, connected=connected, erased=erased, covis10=covis10)


def make_sim3_problem(seed, kind="general", n=300, outlier_frac=0.0, noise_px=0.5, noise_m=0.002, w=752, h=480):
    """Two key frames that see a common cloud, for the Sim3 solver (Sim3Solver) and OptimizeSim3: X1c, X2c [n,3] float32, the matched map
    points in the frame of their own camera, related by X1 = s12 R12 X2 + t12 (ground truth R12, t12, s12) up to noise_m metres of
    Gaussian noise on each map point; obs1, obs2 [n,2] the undistorted key points (the true projections with noise_px pixels of noise),
    octave1, octave2 [n], sigma2_1, sigma2_2 [n] = 1.2^(2 octave), K1 = K2 = fx fy cx cy. kind: "general" (about 20 degrees, s12 = 1.3),
    "fix_scale" (s12 = 1, as with a stereo or RGB-D map) and "small_rotation" (about 0.5 degrees, s12 = 1.05). outlier_frac of the
    correspondences pair a point of camera 1 with the wrong point of camera 2 (true_inlier [n] = 0). numpy only."""
    rng = np.random.Generator(np.random.PCG64(seed + 515151))
    fx, fy, cx, cy = [float(np.float32(v)) for v in (EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"])]
    angle, s12 = dict(general=(np.radians(20.0), 1.3), fix_scale=(np.radians(12.0), 1.0), small_rotation=(np.radians(0.5), 1.05))[kind]
    axis = rng.normal(0, 1, 3); axis /= np.linalg.norm(axis)
    R12 = _rotvec_to_R(axis * angle)
    t12 = np.array([0.6, -0.1, 0.25]) + rng.normal(0, 0.05, 3)
    m = 12 * n + 64
    uv1 = np.stack([rng.uniform(15, w - 15, m), rng.uniform(15, h - 15, m)], 1)
    z = rng.uniform(2.0, 10.0, m)
    X1 = np.stack([(uv1[:, 0] - cx) / fx * z, (uv1[:, 1] - cy) / fy * z, z], 1)
    X2 = (X1 - t12) @ R12 / s12                                    # R12^T (X1 - t12) / s12
    uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    ok = (X2[:, 2] > 1.0) & (uv2[:, 0] > 15) & (uv2[:, 0] < w - 15) & (uv2[:, 1] > 15) & (uv2[:, 1] < h - 15)
    X1, X2, uv1, uv2 = X1[ok][:n], X2[ok][:n], uv1[ok][:n], uv2[ok][:n]
    assert len(X1) == n, "not enough points visible in both cameras"
    true_inlier = np.ones(n, np.uint8)
    out = rng.permutation(n)[:int(round(outlier_frac * n))]
    if len(out):
        other = (out + rng.integers(1, n, len(out))) % n           # never itself
        X2, uv2 = X2.copy(), uv2.copy()
        X2[out], uv2[out] = X2[other], uv2[other]
        true_inlier[out] = 0
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    sig = lambda o: (np.float32(1.2) ** o.astype(np.float32)) ** 2
    return dict(X1c=(X1 + rng.normal(0, noise_m, (n, 3))).astype(np.float32), X2c=(X2 + rng.normal(0, noise_m, (n, 3))).astype(np.float32),
                obs1=(uv1 + rng.normal(0, noise_px, (n, 2))).astype(np.float32), obs2=(uv2 + rng.normal(0, noise_px, (n, 2))).astype(np.float32),
                octave1=o1.astype(np.int32), octave2=o2.astype(np.int32), sigma2_1=sig(o1).astype(np.float32), sigma2_2=sig(o2).astype(np.float32),
                K1=np.array([fx, fy, cx, cy], np.float32), K2=np.array([fx, fy, cx, cy], np.float32), R12=R12, t12=t12, s12=float(s12),
                true_inlier=true_inlier, kind=kind)


def _flip_bits(rng, d, k):
    """A copy of descriptors d [n,32] with k random bit flips per row (a bit may be hit twice)."""
    d = np.array(d, np.uint8, copy=True).reshape(-1, 32)
    for _ in range(k):
        b = rng.integers(0, 256, len(d))
        d[np.arange(len(d)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


def make_sim3_match_problem(seed, n1=1000, n2=1000, n_common=500, fix_scale=False, duplicates=0, siblings=60, cluster=0, n_kf=1, n_extra=300,
                            n_special=12, nlevels=8, w=752, h=480):
    """Two key frames that see a common scene from two maps that differ by a similarity, for the loop-closing matchers (SearchBySim3,
    SearchByProjection(KF, Scw), Fuse(KF, Scw)). Key frame 1 lives in map 1 (metric), key frame 2 in map 2, whose unit is s12 metres (1.3;
    1 with fix_scale) and whose axes are rotated and shifted: X_c1 = s12 R12 X_c2 + t12. Feature i < n_common of both key frames is the
    same scene point. numpy only.

    kf1, kf2: dict(kps, desc, pose12, has_point, pts_f [n,8] from local_points_f32, pts_desc [n,32] = the key point's descriptor with a
    few flipped bits, already [n]). Some common pairs are `already` matched; `siblings` common features of each key frame get a second
    feature a few pixels away with a similar descriptor and a copy of the map point (several candidates under TH_LOW, and one-way matches
    that are not mutual); n_special own-only features per reason get a map point that is behind the other camera, outside its image,
    outside its distance range, or seen from behind (the viewing-angle gate).
    loop: the points of map 2 that Scw [12] projects into key frame 1: pts_f [P,8], pts_desc [P,32], valid [P], feat_taken [n1] (the
    features of key frame 1 that are matched on entry; their points are not valid), source [P] = the feature of key frame 2 or -1.
    duplicates=k appends k noisy copies of loop points whose feature is free, so that several points contend for one feature;
    cluster=c puts c features with near-identical descriptors at one place of key frame 1 and c + 4 copies of one point on them.
    fuse: n_kf key frames near key frame 1 (the first is key frame 1) over the loop points: frames [(kps, desc)], Scw [n_kf,12], valid
    [n_kf,P]."""
    rng = np.random.Generator(np.random.PCG64(seed + 717171))
    fx, fy, cx, cy = [float(np.float32(v)) for v in (EUROC_K["fx"], EUROC_K["fy"], EUROC_K["cx"], EUROC_K["cy"])]
    sf = (np.float32(1.2) ** np.arange(nlevels)).astype(np.float32)
    lsf = np.log(1.2)
    s12 = 1.0 if fix_scale else 1.3
    R1 = _rotvec_to_R(rng.normal(0, 0.03, 3)); t1 = rng.normal(0, 0.05, 3)
    R2 = _rotvec_to_R(np.array([0.02, 0.16, -0.03]) + rng.normal(0, 0.01, 3)) @ R1; t2 = R2 @ (-np.array([0.9, 0.1, 0.3])) + rng.normal(0, 0.02, 3)
    Rd = _rotvec_to_R(rng.normal(0, 0.4, 3)); td = rng.normal(0, 1.0, 3)
    to_w2 = lambda Xw: (Xw @ Rd.T + td) / s12                          # map 2 from the metric world (= map 1)
    R2w = R2 @ Rd.T; t2w = (t2 - R2w @ td) / s12                       # key frame 2 in map 2
    R12 = R1 @ R2.T; t12 = t1 - R12 @ t2
    proj = lambda Xc: np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    inside = lambda uv, z: (z > 0.5) & (uv[:, 0] > 20) & (uv[:, 0] < w - 20) & (uv[:, 1] > 20) & (uv[:, 1] < h - 20)
    cloud = lambda m: np.stack([rng.uniform(-5, 5, m), rng.uniform(-3.5, 3.5, m), rng.uniform(3, 12, m)], 1)
    X = cloud(6 * n_common)
    c1, c2 = X @ R1.T + t1, X @ R2.T + t2
    X = X[inside(proj(c1), c1[:, 2]) & inside(proj(c2), c2[:, 2])][:n_common]
    nc = len(X)
    assert nc == n_common, "not enough points visible in both cameras"
    base = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    coin = lambda: rng.integers(0, 2, nc)

    def view(R, t, n, n_sib, octave_of):
        """A key frame at (R, t) (metric): the common features, then n_sib siblings, then own-only features. octave_of(dist): the octaves
        of the common features from their distances, or None for random ones."""
        Xc = X @ R.T + t
        uv, dist = proj(Xc), np.linalg.norm(Xc, axis=1)
        k = np.zeros(n, KP_NP)
        k["x"][:nc] = uv[:, 0] + rng.normal(0, 0.5, nc); k["y"][:nc] = uv[:, 1] + rng.normal(0, 0.5, nc)
        k["x"][nc:] = rng.uniform(20, w - 20, n - nc); k["y"][nc:] = rng.uniform(20, h - 20, n - nc)
        k["octave"] = rng.integers(0, nlevels, n)
        if octave_of is not None:
            k["octave"][:nc] = np.clip(octave_of(dist), 0, nlevels - 1)
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d[:nc] = _flip_bits(rng, base, 8)
        sib = rng.permutation(nc)[:n_sib]
        js = nc + np.arange(len(sib))
        k["x"][js] = k["x"][sib] + rng.uniform(1.5, 3.5, len(sib)) * rng.choice([-1, 1], len(sib)); k["y"][js] = k["y"][sib] + rng.uniform(-2, 2, len(sib))
        k["octave"][js] = k["octave"][sib]
        d[js] = _flip_bits(rng, base[sib], 20)
        k["angle"] = rng.uniform(0, 360, n); k["size"] = 31 * sf[k["octave"]]; k["class_id"] = -1
        return k, d, dist, sib, js
    # a point of octave o1 at distance d1 is predicted in key frame 2 at level ceil(o1 + log(d1 s12 / d2) / log 1.2), d2 metric; and back
    k1, d1, dist1, sib1, js1 = view(R1, t1, n1, siblings, None)
    k2, d2, dist2, sib2, js2 = view(R2, t2, n2, siblings, lambda dd: np.ceil(k1["octave"][:nc] + np.log(dist1 * s12 / dd) / lsf) - coin())
    pose1 = np.concatenate([R1.ravel(), t1]); pose2 = np.concatenate([R2w.ravel(), t2w])

    def points(k, d, n, pose, Xw_common, sib, js, unit, own_world_from_other_cam, unit_other):
        """The map points of one key frame's features in its own map (unit metres per map unit): the common points, copies for the siblings,
        own-only points on the key point's ray, and the special ones, which are chosen in the OTHER camera's frame (metric)."""
        Rw, tw = pose[:9].reshape(3, 3), pose[9:]
        own = np.arange(nc + len(sib), n)
        Pw = np.zeros((n, 3))
        Pw[:nc] = Xw_common
        Pw[js] = Xw_common[sib] + rng.normal(0, 0.004, (len(sib), 3))
        ray = np.stack([(k["x"][own] - cx) / fx, (k["y"][own] - cy) / fy, np.ones(len(own))], 1) * (rng.uniform(3, 12, len(own)) / unit)[:, None]
        Pw[own] = (ray - tw) @ Rw
        pts_f = local_points_f32(k["octave"], pose, Pw, sf)
        has = np.zeros(n, np.uint8); has[:nc] = 1; has[js] = 1; has[own] = rng.random(len(own)) < 0.6
        sp = own[has[own] == 1][:4 * n_special]
        kinds = np.repeat(np.arange(4), n_special)[:len(sp)]
        zc = rng.uniform(3, 10, len(sp))
        Xo = np.stack([rng.uniform(-0.3, 0.3, len(sp)) * zc, rng.uniform(-0.2, 0.2, len(sp)) * zc, zc], 1)
        Xo[kinds == 0, 2] *= -1                                        # behind the other camera
        Xo[kinds == 1, 0] = zc[kinds == 1] * (w + 60 - cx) / fx        # right of its image
        f = local_points_f32(k["octave"][sp], pose, own_world_from_other_cam(Xo), sf)
        d_other = (np.linalg.norm(Xo, axis=1) / unit_other).astype(np.float32)
        f[:, 6] = d_other * np.float32(0.4); f[:, 7] = d_other * np.float32(1.5)
        f[kinds == 2, 6] = d_other[kinds == 2] * np.float32(2.0); f[kinds == 2, 7] = d_other[kinds == 2] * np.float32(6.0)     # too close
        f[kinds == 3, 3:6] *= -1                                       # the normal points away from both cameras
        pts_f[sp] = f
        return pts_f.astype(np.float32), _flip_bits(rng, d, 3), has, sp, kinds
    pf1, pd1, has1, sp1, kinds1 = points(k1, d1, n1, pose1, X, sib1, js1, 1.0, lambda Xc2: (Xc2 - t2) @ R2, s12)
    pf2, pd2, has2, sp2, kinds2 = points(k2, d2, n2, pose2, to_w2(X), sib2, js2, s12, lambda Xc1: to_w2((Xc1 - t1) @ R1), 1.0)
    truth = np.full(n1, -1, np.int64); truth[:nc] = np.arange(nc)
    al1 = np.zeros(n1, np.uint8); al2 = np.zeros(n2, np.uint8)
    am = rng.permutation(nc)[:max(30, nc // 15)]
    am = am[~np.isin(am, sib1) & ~np.isin(am, sib2)]
    al1[am] = 1; al2[am] = 1

    # ---- the loop points: map 2's points, which Scw = S12 * T2w projects into key frame 1
    Scw = np.concatenate([s12 * R12 @ R2w, (s12 * R12 @ t2w + t12)[:, None]], 1).astype(np.float32).ravel()
    src = np.nonzero(has2)[0]
    lp_f = [pf2[src], local_points_f32(rng.integers(0, nlevels, n_extra), pose2, to_w2(cloud(n_extra)), sf)]
    lp_d = [pd2[src], rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)]
    source = [src, np.full(n_extra, -1, np.int64)]
    free = src[(src < nc) & (al2[src] == 0)]                           # common points whose feature of key frame 1 is free on entry
    if duplicates:
        pick = rng.choice(free, duplicates, replace=duplicates > len(free))
        f = pf2[pick].copy(); f[:, :3] += rng.normal(0, 0.002, (duplicates, 3)).astype(np.float32)
        lp_f.append(f); lp_d.append(_flip_bits(rng, pd2[pick], 3)); source.append(pick)
    if cluster:
        inner = free[(k1["octave"][free] >= min(1, nlevels - 1)) & (k1["octave"][free] <= max(nlevels - 2, 0))]
        j = int(inner[0])                                              # feature j of both key frames
        cl = np.arange(n1 - cluster, n1)                               # the last own-only features of key frame 1 move onto it
        k1["x"][cl] = k1["x"][j] + rng.uniform(-2.5, 2.5, cluster); k1["y"][cl] = k1["y"][j] + rng.uniform(-2.5, 2.5, cluster)
        k1["octave"][cl] = k1["octave"][j]; k1["size"][cl] = k1["size"][j]
        d1[cl] = _flip_bits(rng, np.repeat(d1[j:j + 1], cluster, 0), 4)
        has1[cl] = 0
        lp_f.append(np.repeat(pf2[j:j + 1], cluster + 4, 0)); lp_d.append(_flip_bits(rng, np.repeat(pd2[j:j + 1], cluster + 4, 0), 2))
        source.append(np.full(cluster + 4, j, np.int64))
    lp_f, lp_d, source = np.concatenate(lp_f).astype(np.float32), np.concatenate(lp_d), np.concatenate(source)
    valid = np.ones(len(lp_f), np.uint8)
    valid[(source >= 0) & (al2[np.maximum(source, 0)] == 1)] = 0       # in spAlreadyFound
    valid[rng.random(len(valid)) < 0.02] = 0                           # bad

    # ---- Fuse: key frames near key frame 1, each with its own corrected Scw, over the one list
    frames, Scws, valids = [(k1, d1)], [Scw], [valid.copy()]
    for b in range(1, n_kf):
        Rb = _rotvec_to_R(rng.normal(0, 0.02, 3)) @ R1; tb = t1 + rng.normal(0, 0.08, 3)
        kb, db, _, _, _ = view(Rb, tb, n1, 0, lambda dd: np.ceil(k2["octave"][:nc] - np.log(dd * s12 / dist2) / lsf) - coin())
        Rb2 = Rb @ R2.T; tb2 = tb - Rb2 @ t2
        frames.append((kb, db)); Scws.append(np.concatenate([s12 * Rb2 @ R2w, (s12 * Rb2 @ t2w + tb2)[:, None]], 1).astype(np.float32).ravel())
        v = valid.copy(); v[rng.random(len(v)) < 0.15] = 0             # already in key frame b
        valids.append(v)
    side = lambda k, d, pose, has, pf, pd, al: dict(kps=k, desc=d, pose12=pose.astype(np.float32), has_point=has, pts_f=pf, pts_desc=pd, already=al)
    return dict(kf1=side(k1, d1, pose1, has1, pf1, pd1, al1), kf2=side(k2, d2, pose2, has2, pf2, pd2, al2), truth12=truth,
                R12=R12.astype(np.float32), t12=t12.astype(np.float32), s12=np.float32(s12), intr4=np.array([fx, fy, cx, cy], np.float32), sf=sf,
                bounds4=np.array([0, w, 0, h], np.float32),
                loop=dict(pts_f=lp_f, pts_desc=lp_d, valid=valid, Scw=Scw, feat_taken=al1.copy(), source=source),
                fuse=dict(frames=frames, Scw=np.stack(Scws), valid=np.stack(valids)))


def make_search_init_problem(seed, n_scene=400, shared=0.8, siblings=40, twins=30, wrong_angles=0.1, upper_share=0.2, geometry=False,
                             flow=(14.0, -9.0), w=752, h=480):
    """Two monocular frames of a common scene with a flow between them, for ORBmatcher::SearchForInitialization: kps1 / kps2 (capi.KP_DTYPE
    with octaves and angles), desc1 / desc2 [n,32], prev_matched [n1,2] = the key points of frame 1 (as Tracking sets mvbPrevMatched),
    bounds4, truth12 [n1] (the feature of frame 2 that shows the same scene point, or -1). Frame 1 sees `shared` of the n_scene scene
    features, frame 2 all of them; descriptors differ by 0..30 bit flips, a share by 45..80 (above TH_LOW).
    siblings: extra points of frame 1 beside a scene point with its descriptor but for a few bits: they compete for one feature of frame 2
    (displacements, order dependence). twins: extra features of frame 2 beside a scene feature with its descriptor but for 0..4 bits:
    second-best distances that fail the ratio test, and exact ties. wrong_angles: the share of frame-2 features turned by 60..300 degrees
    (removed by the rotation histogram). upper_share: the share of scene features above pyramid level 0.
    geometry=True: the positions and true matches are those of make_two_view_init_problem(seed, n1=n_scene, n2=n_scene,
    n_matches=shared * n_scene) (K4, R21, t21 in the result) and upper_share only applies to unmatched key points, so that the matches
    initialise. Both frames are shuffled at the end. numpy only."""
    from . import capi
    rng = np.random.Generator(np.random.PCG64(seed + 515151))
    ns = int(round(shared * n_scene))
    extra = {}
    if geometry:
        TV = make_two_view_init_problem(seed, n1=n_scene, n2=n_scene, n_matches=ns, outlier_share=0.0)
        xy1, xy2 = TV["xy1"].astype(np.float64), TV["xy2"].astype(np.float64)
        pair = TV["matches12"].astype(np.int64)
        keep1 = np.nonzero(pair >= 0)[0]                                   # frame 1: the matched key points (siblings are added below)
        xy1, pair = xy1[keep1], pair[keep1]
        extra = dict(K4=TV["K4"], R21=TV["R21"], t21=TV["t21"])
    else:
        xy2 = np.stack([rng.uniform(15, w - 15, n_scene), rng.uniform(15, h - 15, n_scene)], 1)
        pair = rng.permutation(n_scene)[:ns]
        xy1 = xy2[pair] - np.array(flow) + rng.normal(0, 3.0, (ns, 2))
    n2 = len(xy2)
    oct2 = np.where(rng.random(n2) < upper_share, rng.integers(1, 4, n2), 0)
    if geometry:
        oct2[pair] = 0
    ang2 = rng.uniform(0, 360, n2)
    desc2 = rng.integers(0, 256, (n2, 32)).astype(np.uint8)
    # frame 1: the scene point's descriptor with flips, its octave (a few a level off), its angle less a roll
    flips = np.where(rng.random(ns) < 0.12, rng.integers(45, 81, ns), rng.integers(0, 31, ns))
    desc1 = np.stack([_flip_bits(rng, desc2[p], int(k))[0] for p, k in zip(pair, flips)])
    oct1 = oct2[pair].copy()
    off = rng.random(ns) < (0.0 if geometry else 0.03)
    oct1[off] = 1 - np.minimum(oct1[off], 1)
    ang1 = (ang2[pair] - 6.0 + rng.normal(0, 2.0, ns)) % 360.0
    turned = rng.random(ns) < wrong_angles
    ang1[turned] = (ang1[turned] + rng.uniform(60, 300, turned.sum())) % 360.0
    truth = pair.copy()
    # siblings of frame 1
    src = rng.integers(0, ns, siblings)
    s_xy = xy1[src] + rng.uniform(-10, 10, (siblings, 2))
    s_desc = np.stack([_flip_bits(rng, desc1[s], int(k))[0] for s, k in zip(src, rng.integers(0, 7, siblings))]) if siblings else np.zeros((0, 32), np.uint8)
    xy1 = np.concatenate([xy1, s_xy]); desc1 = np.concatenate([desc1, s_desc]); oct1 = np.concatenate([oct1, np.zeros(siblings, np.int64)])
    ang1 = np.concatenate([ang1, (ang1[src] + rng.normal(0, 2.0, siblings)) % 360.0]); truth = np.concatenate([truth, np.full(siblings, -1)])
    # twins of frame 2
    tsrc = pair[rng.integers(0, ns, twins)]
    t_xy = xy2[tsrc] + rng.uniform(-30, 30, (twins, 2))
    t_desc = np.stack([_flip_bits(rng, desc2[s], int(k))[0] for s, k in zip(tsrc, rng.integers(0, 5, twins))]) if twins else np.zeros((0, 32), np.uint8)
    xy2 = np.concatenate([xy2, t_xy]); desc2 = np.concatenate([desc2, t_desc]); oct2 = np.concatenate([oct2, np.zeros(twins, np.int64)])
    ang2 = np.concatenate([ang2, (ang2[tsrc] + rng.normal(0, 2.0, twins)) % 360.0])
    xy1[:, 0] = np.clip(xy1[:, 0], 1, w - 2); xy1[:, 1] = np.clip(xy1[:, 1], 1, h - 2)
    xy2[:, 0] = np.clip(xy2[:, 0], 1, w - 2); xy2[:, 1] = np.clip(xy2[:, 1], 1, h - 2)
    p1, p2 = rng.permutation(len(xy1)), rng.permutation(len(xy2))
    inv2 = np.empty(len(xy2), np.int64); inv2[p2] = np.arange(len(xy2))

    def frame(xy, octave, angle, desc, perm):
        k = np.zeros(len(perm), capi.KP_DTYPE)
        k["x"], k["y"], k["octave"], k["angle"] = xy[perm, 0], xy[perm, 1], octave[perm], angle[perm]
        k["size"] = np.floor(31.0 * 1.2 ** octave[perm]); k["response"] = rng.uniform(20, 120, len(perm)); k["class_id"] = -1
        return k, np.ascontiguousarray(desc[perm])
    k1, d1 = frame(xy1, oct1, ang1, desc1, p1)
    k2, d2 = frame(xy2, oct2, ang2, desc2, p2)
    truth = np.where(truth >= 0, inv2[np.maximum(truth, 0)], -1)[p1].astype(np.int32)
    return dict(kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev_matched=np.stack([k1["x"], k1["y"]], 1).astype(np.float32), truth12=truth,
                bounds4=np.array([0, w, 0, h], np.float32), window_size=100, nnratio=0.9, **extra)


def make_essential_graph_problem(seed, N=20, fix_scale=False, rot_drift=0.004, trans_drift=0.01, scale_drift=0.01, n_corrected=3, n_covis=3,
                                 loop_edges=0, duplicate_pair=False, extra_fixed=(), consistent=False, n_points=0, skip_frac=0.1, radius=5.0, turn=1.0):
    """A closed trajectory for the essential-graph solve (Optimizer::OptimizeEssentialGraph): N key frames on a circle, key frame 0 the
    fixed loop key frame, the odometry between successive key frames drifting in rotation (rot_drift radians per step, a bias plus
    noise), translation (trans_drift of a step) and, without fix_scale, scale (scale_drift per step), so that key frame N - 1 does not
    meet key frame 0 again. The last key frame and n_corrected - 1 of its predecessors carry corrected poses in Scw (the loop's Sim3 for
    the last one, Sic * Scw for the others, as LoopClosing::CorrectLoop propagates it) and their drifted ones in Smeas; every other row
    of Scw is the drifted pose (R, t, 1) and equals its row of Smeas. Edges (vertex 0 = i, vertex 1 = j): a spanning-tree edge (k, k - 1)
    of every key frame, covisibility edges to the predecessors k - 2 .. k - n_covis, `loop_edges` older loop edges between distant key
    frames (all edge_corrected = 0), and LoopConnections edges from every corrected key frame to key frames 0 and 1 (edge_corrected =
    1). duplicate_pair: the pair (N - 1, N - 2) a second time as a LoopConnections edge. extra_fixed: further fixed vertices (with 1
    among them the spanning-tree edge (1, 0) joins two fixed vertices). consistent: no drift and no correction, so every error is zero
    from the start. turn: 1 = the camera follows the tangent (a full revolution of yaw), less = it sways by that many radians. n_points float32 points, each seen from a reference key frame (point_ref), skip_frac of them with point_ref = -1.
    Returns Scw, Smeas [N,8] = r(x y z w) t s, fixed [N], edge_idx [E,2], edge_corrected [E], points [P,3], point_ref [P], fix_scale and
    the drift-free Scw_true. numpy only."""
    rng = np.random.Generator(np.random.PCG64(seed + 626262))
    if consistent:
        rot_drift = trans_drift = scale_drift = 0.0; n_corrected = 0
    n_corrected = min(n_corrected, N - 1)

    def pose(k):                                                   # camera k: on the circle, looking along the tangent, Tcw = (R, t)
        a = 2 * np.pi * k / max(N, 8)
        Rwc = _rotvec_to_R(np.array([0, 0, turn * a if turn == 1.0 else turn * np.sin(a)])) @ _rotvec_to_R(np.array([0.05 * np.sin(3 * a), 0.03 * np.cos(2 * a), 0]))
        twc = np.array([radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(2 * a)])
        return Rwc.T, -Rwc.T @ twc
    true = [pose(k) for k in range(N)]
    bias = rng.normal(0, 1, 3); bias /= max(np.linalg.norm(bias), 1e-12)
    drift = [true[0]]
    sc = 1.0
    for k in range(1, N):
        Rrel = true[k][0] @ true[k - 1][0].T                        # T_k,k-1
        trel = true[k][1] - Rrel @ true[k - 1][1]
        if not fix_scale:
            sc *= 1.0 + scale_drift
        Rrel = _rotvec_to_R(rot_drift * (bias + 0.5 * rng.normal(0, 1, 3))) @ Rrel
        trel = sc * trel * (1 + trans_drift * rng.normal(0, 1, 3))
        drift.append((Rrel @ drift[-1][0], Rrel @ drift[-1][1] + trel))
    row = lambda R, t, s: np.concatenate([_R_to_quat(R), t, [s]])
    Smeas = np.stack([row(R, t, 1.0) for R, t in drift])
    Scw = Smeas.copy()
    if n_corrected:
        c = N - 1
        s = 1.0 if fix_scale else 1.0 / sc                          # the drifted map around the last key frame is sc times too large
        Rc, tc = true[c][0], true[c][1]
        Scw[c] = row(Rc, tc, s)                                     # the loop's Sim3: a world point X of the old map is s Rc X + tc in c
        for i in range(N - n_corrected, N - 1):                     # Sic * Scw with Sic = Tiw Twc of the drifted poses
            Ric = drift[i][0] @ drift[c][0].T
            tic = drift[i][1] - Ric @ drift[c][1]
            Scw[i] = row(Ric @ Rc, Ric @ tc + tic, s)
    fixed = np.zeros(N, np.uint8); fixed[0] = 1
    for v in extra_fixed:
        fixed[int(v)] = 1
    edges, corr = [], []
    corrected = list(range(N - n_corrected, N))
    for k in corrected:                                             # LoopConnections first, as the reference adds them
        for j in (0, 1):
            if j < k and j not in corrected:
                edges.append((k, j)); corr.append(1)
    if duplicate_pair and N >= 3:
        edges.append((N - 1, N - 2)); corr.append(1)
    inserted = set(edges)                                           # sInsertedEdges: a covisibility edge of such a pair is left out
    far = [(k, k - max(7, N // 4)) for k in range(N - 1, 0, -1) if k - max(7, N // 4) >= 0]
    far = [far[q] for q in rng.permutation(len(far))[:loop_edges]] if loop_edges else []
    for k in range(1, N):
        edges.append((k, k - 1)); corr.append(0)
        for (a, b) in far:
            if a == k:
                edges.append((a, b)); corr.append(0)
        for d in range(2, n_covis + 1):
            if k - d >= 0 and (k, k - d) not in inserted:
                edges.append((k, k - d)); corr.append(0)
    P, ref = np.zeros((n_points, 3), np.float32), np.zeros(n_points, np.int32)
    for p in range(n_points):
        r = int(rng.integers(0, N))
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(2, 8)])
        R, t, s = _quat_to_R(Scw[r, :4]), Scw[r, 4:7], Scw[r, 7]
        P[p] = (R.T @ (Xc - t) / s).astype(np.float32)              # the point as the input map holds it: Srw^-1 of its camera position
        ref[p] = -1 if rng.uniform() < skip_frac else r
    return dict(Scw=Scw, Smeas=Smeas, fixed=fixed, edge_idx=np.array(edges, np.int32).reshape(-1, 2), edge_corrected=np.array(corr, np.uint8),
                points=P, point_ref=ref, fix_scale=bool(fix_scale), Scw_true=np.stack([row(R, t, 1.0) for R, t in true]))


def _quat_to_R(q):
    from scipy.spatial.transform import Rotation
    return Rotation.from_quat(q).as_matrix()


def make_culling_problem(seed, n_kf=None, n_cand=None, max_kps=300, min_kps=0, n_pts=None, obs_range=None, stereo=0.3, not_erase=0.1, gap=0.1, same_octave=None, stray=0.02):
    """One stream's snapshot for key-frame culling (the scene dict of viorb_amd/culling.py): a chain of n_kf key frames in time order with the
    current one last, n_pts points each observed by obs_range = (lo, hi) key frames near one another (octaves 0-7 around the point's own,
    a share `stereo` of stereo observations), n_cand candidates in random order whose keypoint tables hold their observations cut to at
    min_kps..max_kps entries, with empty entries, a few entries whose point does not observe the candidate, a few points listed twice and
    depths on both sides of th_depth. `gap`: the share of long intervals (time-gap skips); `not_erase`: the share of mbNotErase;
    `stray`: the share of table entries without an observation (they occur after MapPoint::Replace)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nk = int(n_kf or rng.integers(5, 41))
    nc = min(int(n_cand or rng.integers(1, 31)), nk - 1)
    npt = int(n_pts or rng.integers(50, 601))
    lo, hi = obs_range or [(1, 12), (4, 6), (5, 12), (4, 5)][int(rng.integers(0, 4))]
    same = float(rng.choice([0.5, 0.9, 1.0])) if same_octave is None else same_octave
    dt = np.where(rng.random(nk) < gap, rng.uniform(0.3, 0.6, nk), rng.uniform(0.03, 0.15, nk))
    t = 100.0 + np.cumsum(dt)
    s = dict(cur=nk - 1, vins_inited=bool(rng.random() < 0.4), th_depth=40.0)
    flags = np.where(rng.random(nk) < not_erase, 2, 0).astype(np.uint8)
    if rng.random() < 0.5:
        flags[0] |= 1
    s["kf_flags"], s["kf_time"] = flags, t
    s["kf_prev"], s["kf_next"] = np.arange(-1, nk - 1, dtype=np.int32), np.concatenate([np.arange(1, nk), [-1]]).astype(np.int32)
    per_kf = [[] for _ in range(nk)]                       # (point, octave) of every observation of a key frame
    obs_start, obs, nobs = [0], [], []
    for p in range(npt):
        k = min(int(rng.integers(lo, hi + 1)), nk)
        c = int(rng.integers(0, nk))
        w0 = min(max(c - k, 0), max(nk - 2 * k, 0))
        slots = np.sort(rng.choice(np.arange(w0, min(w0 + 2 * k, nk)), size=k, replace=False))
        base = int(rng.integers(0, 8))
        n = 0
        for sl in slots:
            o = base if rng.random() < same else int(np.clip(base + rng.integers(-2, 3), 0, 7))
            st = bool(rng.random() < stereo)
            obs.append((int(sl) & 0xffff) | (o << 16) | ((1 << 24) if st else 0))
            per_kf[int(sl)].append((p, o))
            n += 2 if st else 1
        obs_start.append(len(obs)); nobs.append(n)
    s["pt_nobs"], s["pt_bad"] = np.array(nobs, np.int32), (rng.random(npt) < 0.02).astype(np.uint8)
    s["obs_start"], s["obs"] = np.array(obs_start, np.int32), np.array(obs, np.uint32)
    cand = rng.permutation(nk - 1)[:nc]
    kp_start, point, octave = [0], [], []
    for c in cand:
        rows = [per_kf[int(c)][i] for i in rng.permutation(len(per_kf[int(c)]))][:int(rng.integers(min_kps, max_kps + 1))]
        for (p, o) in rows:
            r = rng.random()
            if r < 0.15 and len(point) - kp_start[-1] < max_kps - 1:
                point.append(-1); octave.append(int(rng.integers(0, 8)))
            elif r < 0.15 + stray and len(point) - kp_start[-1] < max_kps - 1:       # a table entry whose point has no observation of this key frame
                point.append(int(rng.integers(0, npt))); octave.append(int(rng.integers(0, 8)))
            elif r < 0.16 + stray and len(point) - kp_start[-1] < max_kps - 1:       # the point at two keypoints
                point.append(p); octave.append(int(np.clip(o + 1, 0, 7)))
            point.append(p); octave.append(o)
        del point[kp_start[-1] + max_kps:], octave[kp_start[-1] + max_kps:]
        kp_start.append(len(point))
    n = len(point)
    depth = np.where(rng.random(n) < 0.05, rng.uniform(40, 80, n), rng.uniform(0.5, 40, n))
    depth[rng.random(n) < 0.02] = -1.0
    s["cand_kf"], s["kp_start"] = cand.astype(np.int32), np.array(kp_start, np.int32)
    s["kp_point"], s["kp_octave"], s["kp_depth"] = np.array(point, np.int32), np.array(octave, np.uint8), depth.astype(np.float32)
    return s


def make_reloc_problem(seed, n_feat=1000, n_pts=1000, n_cand=1, shared=0.7, n_bow=80, n_inliers=40, nlevels=8, w=752, h=480):
    """A lost frame of n_feat features and n_cand candidate key frames of n_pts map points each, as Tracking::Relocalization meets them
    after PnPsolver::iterate: a share `shared` of each candidate's points is seen in the frame (a feature near the projection, a
    descriptor some bits away), n_bow of them are SearchByBoW matches and n_inliers of those RANSAC inliers, so that the cascade's first
    solve leaves between 10 and 50 good points, the coarse search runs and the second solve decides. dict(kps, desc, intr4, sf, bounds4, hyps): a hypothesis is
    dict(pose12, kf_angle, kf_valid, kf_found, feat_taken, pts_f, pts_desc, bow_match, inlier), indexed by key-frame feature."""
    from .capi import KP_DTYPE
    rng = np.random.default_rng(seed)
    f32 = np.float32
    intr4 = np.array([458.654, 457.296, 367.215, 248.375], f32)
    sf = (f32(1.2) ** np.arange(nlevels)).astype(f32)
    R = _rotvec_to_R(rng.normal(0, 0.3, 3)); t = rng.normal(0, 1.0, 3)
    kps = np.zeros(n_feat, KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(8, w - 12, n_feat), rng.uniform(8, h - 12, n_feat)
    kps["octave"] = np.minimum(rng.geometric(0.35, n_feat) - 1, nlevels - 1)
    kps["angle"], kps["size"], kps["response"] = rng.uniform(0, 359.9, n_feat), 31 * sf[kps["octave"]], 50
    desc = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    hyps = []
    for c in range(n_cand):
        seen = rng.permutation(n_feat)[:min(int(shared * n_pts), n_feat)]
        pts_f, pts_desc, ang = np.zeros((n_pts, 8), f32), rng.integers(0, 256, (n_pts, 32), dtype=np.uint8), rng.uniform(0, 359.9, n_pts).astype(f32)
        z = rng.uniform(2, 10, n_pts)
        u, v = rng.uniform(0, w, n_pts), rng.uniform(0, h, n_pts)
        lvl = rng.integers(0, nlevels, n_pts)
        u[:len(seen)], v[:len(seen)] = kps["x"][seen] + rng.normal(0, 0.7, len(seen)), kps["y"][seen] + rng.normal(0, 0.7, len(seen))
        lvl[:len(seen)] = kps["octave"][seen]
        Xc = np.stack([(u - intr4[2]) / intr4[0] * z, (v - intr4[3]) / intr4[1] * z, z], 1)
        Xw = (Xc - t) @ R                                          # R^T (Xc - t), row-wise
        dist = np.linalg.norm(Xc, axis=1)
        pts_f[:, :3] = Xw
        pts_f[:, 7] = dist * 1.2 ** (lvl - 0.5); pts_f[:, 6] = pts_f[:, 7] / 1.2 ** (nlevels - 1)
        for k, f in enumerate(seen):
            pts_desc[k] = _flip_bits(rng, desc[f], int(rng.integers(0, 45)))
            ang[k] = (kps["angle"][f] + 30.0 + rng.normal(0, 4)) % 360.0
        order = rng.permutation(n_pts)                               # the key frame's own feature order
        inv = np.argsort(order)
        pts_f, pts_desc, ang = pts_f[order], pts_desc[order], ang[order]
        bow, inl = np.full(n_feat, -1, np.int32), np.zeros(n_feat, np.uint8)
        for k in range(min(n_bow, len(seen))):
            bow[seen[k]] = inv[k]
            inl[seen[k]] = k < n_inliers
        dR = _rotvec_to_R(rng.normal(0, 0.002, 3))
        pose = np.concatenate([(dR @ R).ravel(), dR @ t + rng.normal(0, 0.01, 3)]).astype(f32)
        found = np.zeros(n_pts, np.uint8); found[bow[inl != 0]] = 1
        hyps.append(dict(pose12=pose, kf_angle=ang, kf_valid=(rng.uniform(size=n_pts) > 0.03).astype(np.uint8), kf_found=found, feat_taken=inl.copy(),
                         pts_f=pts_f, pts_desc=pts_desc, bow_match=bow, inlier=inl, frame=0))
    return dict(kps=kps, desc=desc, intr4=intr4, sf=sf, bounds4=np.array([0, w, 0, h], f32), hyps=hyps)
