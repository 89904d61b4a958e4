"""Seeded synthetic stereo SEQUENCES with exact ground truth (the inputs of the VO loop, vo.py).

A piecewise-planar scene seen by a KITTI-like stereo rig driving forward:

    ground plane (y = +1.65 m, camera y axis down), two side walls (x = +-8 m), a back wall (z = 100 m) and fronto-parallel
    billboards at 5-40 m, each plane textured with synth's value noise + rectangles (one texture per plane, texels of a
    fixed size in metres).

Rendering is exact per pixel: the ray through the pixel centre (OpenCV convention, pixel (j, i) at (x, y) = (j, i)) is
intersected with every plane (the inverse homography of the plane), the nearest hit in front of the camera wins and its
texture is sampled bilinearly; no noise is added, so the images are a pure function of the scene and the pose. The right
camera sits bf / fx metres along the left camera's +x axis (the KITTI rig). The motion is a smooth forward drive with a
slight yaw; at the default speed the flow of the nearest visible surfaces stays within a few tens of pixels, inside the
reach of the 3-level LK pyramid the tracker uses. All random draws come from synth.Stream (splitmix64), so a seed gives the
same bytes on every machine.
"""
import numpy as np

from .synth import Stream, _draw, _value_noise

KITTI_K = (718.856, 718.856, 607.1928, 185.2157)
KITTI_BF = float(np.float32(0.573 * 718.856))   # test/test_vo.cpp:633-635,800: d * fx
CAM_HEIGHT = 1.65


def _texture(st, tw, th):
    img = _value_noise(st, tw, th, cell=24)
    n = max(tw * th // 400, 1)
    cx = st.uniform(n, 0, tw); cy = st.uniform(n, 0, th)
    hw = st.uniform(n, 3, 14); hh = st.uniform(n, 3, 14)
    rot = st.uniform(n) < 0.5
    ang = np.where(rot, st.uniform(n, 0.15, np.pi / 2 - 0.15), 0.0)
    delta = st.uniform(n, 40, 120) * np.where(st.uniform(n) < 0.5, -1.0, 1.0)
    for i in range(n):
        _draw(img, cx[i], cy[i], hw[i], hh[i], float(ang[i]), delta[i])
    return np.clip(img, 0, 255).astype(np.float32)


def _plane(st, origin, a, b, ea, eb, texel):
    """Rectangle origin + s a + t b, s in [0, ea), t in [0, eb) metres, textured at `texel` metres per texel."""
    tw, th = int(np.ceil(ea / texel)) + 1, int(np.ceil(eb / texel)) + 1
    return dict(o=np.asarray(origin, np.float64), a=np.asarray(a, np.float64), b=np.asarray(b, np.float64), ea=float(ea),
                eb=float(eb), texel=float(texel), tex=_texture(st, tw, th))


def scene(seed, billboards=10):
    """The planes of sequence `seed`: ground, left wall, right wall, back wall, then the billboards."""
    st = Stream(0x5E0_0000 + int(seed))
    planes = [
        _plane(st, (-10.0, CAM_HEIGHT, -5.0), (1, 0, 0), (0, 0, 1), 20.0, 110.0, 0.04),   # ground (y down)
        _plane(st, (-8.0, -4.0, -5.0), (0, 0, 1), (0, 1, 0), 110.0, 4.0 + CAM_HEIGHT, 0.04),   # left wall
        _plane(st, (8.0, -4.0, -5.0), (0, 0, 1), (0, 1, 0), 110.0, 4.0 + CAM_HEIGHT, 0.04),    # right wall
        _plane(st, (-60.0, -30.0, 100.0), (1, 0, 0), (0, 1, 0), 120.0, 30.0 + CAM_HEIGHT, 0.1),   # back wall
    ]
    z = st.uniform(billboards, 5.0, 40.0)
    w = st.uniform(billboards, 1.5, 3.5)
    # beside the road (centre 3.5-6.5 m to either side): the drive never passes through one
    x = st.uniform(billboards, 3.5, 6.5) * np.where(st.uniform(billboards) < 0.5, -1.0, 1.0)
    h = st.uniform(billboards, 1.0, 2.5)
    top = st.uniform(billboards, -2.0, 0.0)
    for i in range(billboards):   # fronto-parallel: s along +x, t along +y (down)
        planes.append(_plane(st, (x[i] - w[i] / 2, top[i], z[i]), (1, 0, 0), (0, 1, 0), w[i], h[i], 0.01))
    return planes


def trajectory(seed, T, speed=0.5, yaw_amp=0.04, period=40.0):
    """Camera centres and yaws of frames 0..T-1: forward drive along +z with a slight sinusoidal yaw -> Tcw [T, 4, 4] float64."""
    st = Stream(0x7A0_0000 + int(seed))
    phase = float(st.uniform(1, 0.0, 2 * np.pi)[0])
    x0 = float(st.uniform(1, -1.0, 1.0)[0])
    out = np.zeros((T, 4, 4))
    c = np.array([x0, 0.0, 0.0])
    for t in range(T):
        yaw = yaw_amp * np.sin(2 * np.pi * t / period + phase)
        cy_, sy_ = np.cos(yaw), np.sin(yaw)
        Rwc = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
        out[t, :3, :3] = Rwc.T
        out[t, :3, 3] = -Rwc.T @ c
        out[t, 3, 3] = 1.0
        c = c + speed * Rwc[:, 2]
    return out


def _bbox(p, Tcw, K, width, height):
    """Pixel box (y0, y1, x0, x1) that holds the plane's image; None when it is behind the camera; the whole image when
    the plane crosses the camera's z = 0.1 plane (ground, walls)."""
    fx, fy, cx, cy = K
    corners = [p["o"] + i * p["ea"] * p["a"] + j * p["eb"] * p["b"] for i in (0, 1) for j in (0, 1)]
    Xc = np.array([Tcw[:3, :3] @ c + Tcw[:3, 3] for c in corners])
    if (Xc[:, 2] <= 0.1).all():
        return None
    if (Xc[:, 2] <= 0.1).any():
        return 0, height, 0, width
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    v = fy * Xc[:, 1] / Xc[:, 2] + cy
    x0, x1 = max(int(np.floor(u.min())) - 1, 0), min(int(np.ceil(u.max())) + 2, width)
    y0, y1 = max(int(np.floor(v.min())) - 1, 0), min(int(np.ceil(v.max())) + 2, height)
    if x1 <= x0 or y1 <= y0:
        return None
    return y0, y1, x0, x1


def render(planes, Tcw, width, height, K=KITTI_K, aux=False):
    """u8 image of the scene seen from Tcw (4x4, world -> camera). aux=True also returns dict(depth, plane, s, t) per pixel
    (plane -1 / depth inf where no plane is hit)."""
    fx, fy, cx, cy = K
    Tcw = np.asarray(Tcw, np.float64)
    Rwc = Tcw[:3, :3].T
    C = -Rwc @ Tcw[:3, 3]
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)     # camera rays with z = 1: lambda = depth
    dw = dc @ Rwc.T
    depth = np.full((height, width), np.inf)
    pid = np.full((height, width), -1, np.int32)
    S = np.zeros((height, width)); Tt = np.zeros((height, width))
    for k, p in enumerate(planes):
        box = _bbox(p, Tcw, K, width, height)
        if box is None:
            continue
        y0, y1, x0, x1 = box
        d = dw[y0:y1, x0:x1]
        n = np.cross(p["a"], p["b"])
        den = d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = ((p["o"] - C) @ n) / den
            X = C + lam[..., None] * d - p["o"]
        s = X @ p["a"]; t = X @ p["b"]
        dep = depth[y0:y1, x0:x1]
        with np.errstate(invalid="ignore"):
            hit = np.isfinite(lam) & (lam > 0.1) & (s >= 0) & (s < p["ea"]) & (t >= 0) & (t < p["eb"]) & (lam < dep)
        dep[hit] = lam[hit]; pid[y0:y1, x0:x1][hit] = k; S[y0:y1, x0:x1][hit] = s[hit]; Tt[y0:y1, x0:x1][hit] = t[hit]
    img = np.zeros((height, width), np.float32)
    for k, p in enumerate(planes):
        m = pid == k
        if not m.any():
            continue
        tex = p["tex"]
        th, tw = tex.shape
        x = np.clip(S[m] / p["texel"] - 0.5, 0, tw - 1.0001)
        y = np.clip(Tt[m] / p["texel"] - 0.5, 0, th - 1.0001)
        x0 = x.astype(np.int64); y0 = y.astype(np.int64)
        fx_, fy_ = x - x0, y - y0
        val = (tex[y0, x0] * (1 - fx_) * (1 - fy_) + tex[y0, x0 + 1] * fx_ * (1 - fy_) + tex[y0 + 1, x0] * (1 - fx_) * fy_ +
               tex[y0 + 1, x0 + 1] * fx_ * fy_)
        img[m] = val
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if aux:
        return out, dict(depth=depth, plane=pid, s=S, t=Tt)
    return out


def right_pose(Tcw, bf=KITTI_BF, fx=KITTI_K[0]):
    """Tcw of the right camera: centre bf / fx metres along the left camera's +x axis."""
    T = np.array(Tcw, np.float64)
    T[0, 3] -= bf / fx
    return T


def sequence(seed, T, width=1241, height=376, K=KITTI_K, bf=KITTI_BF, speed=0.5, yaw_amp=0.04, billboards=10):
    """Stereo sequence `seed` of T frames -> (left [T, H, W] u8, right [T, H, W] u8, Tcw_gt [T, 4, 4] float32)."""
    planes = scene(seed, billboards)
    Tcw = trajectory(seed, T, speed, yaw_amp)
    left = np.zeros((T, height, width), np.uint8)
    right = np.zeros((T, height, width), np.uint8)
    for t in range(T):
        left[t] = render(planes, Tcw[t], width, height, K)
        right[t] = render(planes, right_pose(Tcw[t], bf, K[0]), width, height, K)
    return left, right, Tcw.astype(np.float32)
