"""General cameras for the projection tests: rotated, off the origin, fx != fy, principal point off the image centre.

Under the identity view every product with a view-matrix entry is a product with 0 or 1, which is exact: a transposed read of the
view rotation, fx in the place of fy, x and y exchanged in the fov clamp, an SH direction taken from the view-space point or a depth
read from the wrong column all leave an identity-view test untouched.  The cameras here make every one of those terms non-trivial;
tests/test_camera_general_host.py anchors the fp64 C oracle under them (equivariance under a rigid motion, the autograd twin,
finite differences, mutated cameras), tests/test_gpu_camera_general.py then holds the HIP paths against that oracle.

Numpy only.  ``cameras(W, H)`` -> name -> camera dict of ``sings_amd.camera.make_camera`` plus the numbers it was made from;
``scene(cam, N, deg, seed)`` -> the keys of ``sings_amd.scene.synthetic_scene`` for that camera.
"""
import math

import numpy as np

import sh_case
from sings_amd.camera import get_projection_matrix, get_projection_matrix_center, make_camera

NAMES = ("identity", "yaw", "roll", "generic", "offcentre", "orbit1", "orbit3")
GENERAL = NAMES[1:]
CLAMP_MIN = dict(x=32, y=32, xy=16)            # the smallest fov-clamp groups a scene may carry (beyond 1.3 tanfov in x, y, both)
SH_SHIFT = np.array([0.7, -1.1, 0.4])

# (camera, N, W, H, degree, seed) of every oracle-compared drop-in scene of tests/test_gpu_camera_general.py; the host file
# checks the borderline share, the visible share and the clamp groups of each.  ``roll`` gets W != H on purpose.
FORWARD = [(n, 2000, 128, 96, 3, 31) for n in NAMES]
BACKWARD = [(n, 3000, 160, 128, 3, 32) for n in NAMES]
PRECOMP = [("generic", 1500, 96, 80, 0, 33)]
AUX = [("generic", 2000, 128, 96, 3, 34)]
RENDER = [("orbit1", 2500, 160, 96, 2, 35), ("orbit3", 2500, 160, 96, 2, 35)]
GPU_SCENES = FORWARD + BACKWARD + PRECOMP + AUX + RENDER


def axis_angle(axis, angle):
    """Rotation matrix (fp64) of `angle` rad about `axis` (Rodrigues)."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def axis_angle_quat(axis, angle):
    """(w, x, y, z) of the same rotation."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * a])


def quat_left(q):
    """L(q) with q (x) p = L(q) p, quaternions (w, x, y, z)."""
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]], np.float64)


def rotmat_to_quat(R):
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix (fp64; largest-component branch)."""
    R = np.asarray(R, np.float64)
    tr = np.trace(R)
    cand = np.array([1 + tr, 1 + 2 * R[0, 0] - tr, 1 + 2 * R[1, 1] - tr, 1 + 2 * R[2, 2] - tr])
    k = int(cand.argmax())
    s = 2 * math.sqrt(cand[k])
    if k == 0:
        q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4]
    q = np.array(q)
    return q if q[0] >= 0 else -q


def _camera(name, R, t, fx, fy, cx, cy, W, H):
    """p_view = R p_world + t (column vectors).  The dict of make_camera, plus what it was made from (fp64)."""
    E = np.eye(4); E[:3, :3] = R; E[:3, 3] = t
    cam = make_camera(E, fx, fy, cx, cy, W, H)
    centred = abs(cx - W / 2) < 1e-6 and abs(cy - H / 2) < 1e-6          # the branch make_camera takes
    P = get_projection_matrix(0.01, 100.0, cam["fovx"], cam["fovy"]) if centred else \
        get_projection_matrix_center(0.01, 100.0, fx, fy, cx, cy, W, H)
    cam.update(P=P.astype(np.float64), name=name, extrinsic=E, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), W=int(W), H=int(H),
               tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5))
    return cam


def cameras(W, H):
    from sings_amd.camera import fov2focal, get_rotating_camera
    f = 1.2 * W                                                       # the focal length of synthetic_scene
    Rg = axis_angle((0.48, -0.62, 0.62), 0.9); tg = (0.4, -0.3, 0.7)
    out = {
        "identity": _camera("identity", np.eye(3), np.zeros(3), f, f, W / 2, H / 2, W, H),
        "yaw": _camera("yaw", axis_angle((0, 1, 0), math.radians(35.0)), (0.6, -0.25, 0.9), f, f, W / 2, H / 2, W, H),
        "roll": _camera("roll", axis_angle((0, 0, 1), math.radians(100.0)), (-0.2, 0.35, 0.5), f, f, W / 2, H / 2, W, H),
        "generic": _camera("generic", Rg, tg, f, 1.2 * f, W / 2, H / 2, W, H),
        "offcentre": _camera("offcentre", Rg, tg, f, 1.2 * f, W / 2 + 7.5, H / 2 - 4.25, W, H),
    }
    orbit = get_rotating_camera(img_size=(H, W), device="cpu", nframes=5)
    for i in (1, 3):
        c = orbit[i]
        E = c["world_view_transform"].numpy().astype(np.float64).T      # world_view_transform is the transposed extrinsic
        # the orbit cameras have fovx = fovy = fov on a W x H image: fx = W / (2 tan), fy = H / (2 tan)
        out[f"orbit{i}"] = _camera(f"orbit{i}", E[:3, :3], E[:3, 3], fov2focal(c["fovx"], W), fov2focal(c["fovy"], H), W / 2, H / 2, W, H)
    assert tuple(out) == NAMES
    return out


def retarget(cam, like):
    """The extrinsic of `cam` with the intrinsics and image size of `like` (a K-camera launch has one tanfov pair)."""
    E = cam["extrinsic"]
    return _camera(cam["name"], E[:3, :3], E[:3, 3], like["fx"], like["fy"], like["cx"], like["cy"], like["W"], like["H"])


def matrices64(cam):
    """(viewmatrix, projmatrix, campos) in fp64 from the exact extrinsic: the fp32 matrices of the camera dict are a rounded
    rotation, which an fp64 equivariance check would see at 1e-8.  The projection P is the camera's own (fp32 values)."""
    E = cam["extrinsic"]
    view = E.T.copy()
    return view, view @ cam["P"].T, -E[:3, :3].T @ E[:3, 3]


def to_view(cam, means):
    """World -> view space in fp64."""
    E = cam["extrinsic"]
    return np.asarray(means, np.float64) @ E[:3, :3].T + E[:3, 3]


def clamp_flags(cam, means):
    """(x beyond the limit, y beyond the limit) of the fov clamp 1.3 tanfov, per Gaussian in front of the near plane."""
    t = to_view(cam, means)
    front = t[:, 2] > 0.2
    z = np.where(front, t[:, 2], 1.0)
    return front & (np.abs(t[:, 0] / z) > 1.3 * cam["tanfovx"]), front & (np.abs(t[:, 1] / z) > 1.3 * cam["tanfovy"])


def _clamp_population(rs, cam, n_x, n_y, n_xy):
    """View-space splats whose CENTRE lies beyond 1.3 tanfov (x only, y only, both) and whose 3-sigma radius reaches well into
    the image: sigma = 1 / 1.6 of the centre's distance from the image, so the nearest image pixels see alpha = o exp(-1.28)."""
    W, H, fx, fy, tx, ty = cam["W"], cam["H"], cam["fx"], cam["fy"], cam["tanfovx"], cam["tanfovy"]
    n = n_x + n_y + n_xy
    kind = np.concatenate([np.zeros(n_x, int), np.ones(n_y, int), np.full(n_xy, 2)])
    out_r = rs.uniform(1.36, 1.55, (n, 2)) * np.where(rs.rand(n, 2) < 0.5, -1.0, 1.0)       # beyond the limit, either side
    in_r = rs.uniform(-0.7, 0.7, (n, 2))
    rx = np.where(kind != 1, out_r[:, 0], in_r[:, 0])
    ry = np.where(kind != 0, out_r[:, 1], in_r[:, 1])
    z = rs.uniform(3.0, 8.0, n)
    means = np.stack([rx * tx * z, ry * ty * z, z], 1)
    dx = np.maximum(np.abs(rx) - 1.0, 0.0) * W / 2; dy = np.maximum(np.abs(ry) - 1.0, 0.0) * H / 2
    sigma_px = np.hypot(dx, dy) / 1.6
    s = (sigma_px * z / min(fx, fy))[:, None] * np.exp(rs.normal(0, 0.15, (n, 3)))
    q = rs.normal(0, 1, (n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    opac = rs.uniform(0.25, 0.6, (n, 1))
    return means, s, q, opac, kind


def scene(cam, N, deg, seed, M=16, clamp=(48, 48, 24), unit_quats=False):
    """N Gaussians drawn in VIEW space exactly as synthetic_scene draws them (same visible share for every camera, anisotropic
    scales, 10 % non-unit quaternions unless `unit_quats`), then `clamp` = (x, y, both) fov-clamp splats; means and rotations are
    moved to world space by the inverse extrinsic in fp64.  Keys of synthetic_scene, plus ``clamp_kind`` [N_total]: -1 plain,
    0 / 1 / 2 beyond the limit in x / y / both."""
    rs = np.random.RandomState(seed)
    W, H, fx, tanfovx, tanfovy = cam["W"], cam["H"], cam["fx"], cam["tanfovx"], cam["tanfovy"]
    z = rs.uniform(2, 10, N)
    u = rs.uniform(-1, 1, N); v = rs.uniform(-1, 1, N)
    x = u * 1.1 * z * tanfovx; y = v * 1.1 * z * tanfovy
    near = rs.rand(N) < 0.01
    z = np.where(near, rs.uniform(-1, 0.2, N), z)
    means_v = np.stack([x, y, z], 1)
    sigma_px = np.exp(rs.normal(math.log(2.0), 0.5, N))
    s = (sigma_px * np.abs(z) / fx)[:, None] * np.exp(rs.normal(0, 0.3, (N, 3)))
    q = rs.normal(0, 1, (N, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    nonunit = rs.rand(N) < 0.10
    stretch = 1 + 0.01 * rs.normal(0, 1, (N, 1))
    opac = rs.uniform(0.05, 1.0, (N, 1))
    kind = np.full(N, -1)
    if sum(clamp):
        cm, cs, cq, co, ck = _clamp_population(rs, cam, *clamp)
        means_v = np.concatenate([means_v, cm]); s = np.concatenate([s, cs]); q = np.concatenate([q, cq])
        opac = np.concatenate([opac, co]); kind = np.concatenate([kind, ck])
        nonunit = np.concatenate([nonunit, np.zeros(len(ck), bool)]); stretch = np.concatenate([stretch, np.ones((len(ck), 1))])
    Nt = len(kind)
    # world space: p_w = R^T (p_v - t), R_w = R^T R_v -> q_w = conj(q_E) (x) q_v; the norm of a non-unit quaternion goes on afterwards
    E = cam["extrinsic"]; R, t = E[:3, :3], E[:3, 3]
    means_w = (means_v - t) @ R
    qE = rotmat_to_quat(R)
    q_w = q @ quat_left(qE * np.array([1.0, -1.0, -1.0, -1.0])).T
    if not unit_quats:
        q_w = np.where(nonunit[:, None], q_w * stretch, q_w)
    shs = np.concatenate([rs.normal(0, 1, (Nt, 1, 3)), rs.normal(0, 0.15, (Nt, M - 1, 3))], 1).astype(np.float32)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    dL = rs.normal(0, 1, (3, H, W)).astype(np.float32)
    return dict(N=Nt, W=W, H=H, sh_degree=deg, tanfovx=tanfovx, tanfovy=tanfovy, fovx=cam["fovx"], fovy=cam["fovy"],
                viewmatrix=cam["world_view_transform"], projmatrix=cam["full_proj_transform"], campos=cam["camera_center"],
                means3D=means_w.astype(np.float32), scales=s.astype(np.float32), rotations=q_w.astype(np.float32),
                opacities=opac.astype(np.float32), shs=shs, bg=bg, dL_dimage=dL, clamp_kind=kind, cam=cam)


def gpu_scene(name, N, W, H, deg, seed, **kw):
    return scene(cameras(W, H)[name], N, deg, seed, **kw)


def shifted_sh_groups(shift=SH_SHIFT):
    """The six groups of sh_case with the Gaussians AND the camera centre moved by `shift` (the view translation follows): the
    directions mean - campos, hence the expected colours, are those of sh_case; a direction taken from the view-space point, or
    from the mean alone, is not."""
    fov = 2.0 * np.arctan(sh_case.TANFOV)
    P = get_projection_matrix(0.01, 100.0, fov, fov).astype(np.float64)
    out = []
    for g in sh_case.groups():
        view = g["viewmatrix"].astype(np.float64).copy()
        view[3, :3] = -(np.asarray(shift, np.float64) @ view[:3, :3])     # row-vector convention: p_view = (p - shift) @ view[:3,:3]
        g = dict(g)
        g["means3D"] = (g["means3D"].astype(np.float64) + shift).astype(np.float32)
        g["viewmatrix"] = view.astype(np.float32)
        g["projmatrix"] = (view @ P.T).astype(np.float32)
        g["campos"] = np.asarray(shift, np.float32)
        out.append(g)
    return out
