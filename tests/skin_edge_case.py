"""The cases of the fused skinning kernels' edge tests (no GPU): tests/test_skin_edge_cases_host.py proves from the oracles alone
that they test what they claim, tests/test_gpu_skin_edges.py runs them on the device.

What the kernels of sings_amd/csrc/sg_skin.hip (weight staging: sg_skin.h) branch on: the joint count J -- chunks of 16 joints (``(J + 15) >> 4``), k-steps of
4 (``(J + 3) >> 2``), a float4 staging path for J % 4 == 0 and a scalar one otherwise, the K-frame backward's dynamic LDS of
22528 + 1024 J bytes (past 64 KiB from J = 43) -- and where the Gaussian count P falls inside a 64-lane wave and a 256-thread
workgroup.  The C ABI takes 1 <= J <= 64 and any P >= 1; ``SINGLE`` and ``FRAMES`` walk those edges, each list stated case by
case (no cross product).

``scene`` follows tests/test_gpu_skinned._scene (random rigid A, sparse weights rand**6 thresholded at 0.1 and renormalised,
smpl_scale, transl, degree-3 SH with M = 16, random dL) with three changes: a 64 x 48 camera with fx = fy = 375 (3072 pixels: the
raster oracle takes milliseconds), scales x 4 (a few hundred Gaussians still cover pixels), and the 0.3 bonus of Gaussian i on
joint perm[i % J], so that every joint carries weight whenever P >= J.

Seeds are fixed here; a seed that missed a condition of the host file was replaced (see ``_SINGLE_SEEDS``).

Tolerance headroom of test_gpu_skin_edges.py (b), measured on the committed cases (all 104 posed frames) by
test_skin_edge_cases_host.py::test_fp32_restatement_stays_within_a_quarter_of_the_gpu_bar: the fp32 restatement's gradients
against the fp64 restatement's, random upstream gradients on the posed means, quaternions and scales, reach at most 0.227 of the
bar of (b) (tests/test_gpu_skinned._close's pairs x 0.1 = 0.023 of the pairs themselves).  The worst array is the canonical
rotation in 6-D form (Gram-Schmidt of a random row is ill-conditioned when its halves are nearly parallel: 0.089 with 3 x 3
matrices); the others: xyz_canon 0.114, scales 0.001, A 0.007, transl 0.003.  LAB.md, "Fused skinning kernels at the edges",
has the device's figures next to these.
"""
import numpy as np
import torch

from oracle import lbs_oracle as lo

M = 16
ROTS = ("6d", "mat", "iso")
# (b)'s bar: test_gpu_skinned._close's pairs (5e-4, 5e-6) and, for A / transl, (2e-3, 2e-4), times 0.1
BAR_FACTOR = 0.1
BAR = dict(xyz_canon=(5e-5, 5e-7), rot_canon=(5e-5, 5e-7), scales=(5e-5, 5e-7), A=(2e-4, 2e-5), transl=(2e-4, 2e-5))


def _camera(W, H):
    from sings_amd.camera import make_camera
    return make_camera(np.eye(4, dtype=np.float32), 375.0, 375.0, W / 2, H / 2, W, H)


def scene(P, J, seed, rot, W=64, H=48, K=None):
    """-> dict of numpy arrays.  ``rot``: "6d" (``rot_in`` [P,6]: what the kernels are handed), "mat" (``rot_in`` [P,3,3], the
    matrices of those rows), "iso" (``rot_in`` None, isotropic scales).  ``Rc`` [P,3,3] | None: the canonical rotation matrices.
    ``K`` None: one frame (``A`` [J,4,4], ``transl`` [3], ``dL`` [3,H,W]); else ``A`` [K,J,4,4], ``transl`` [K,3], ``dL`` [K,3,H,W],
    frame 0 being the single-frame scene of the same seed and the other frames' A and transl drawn independently."""
    assert rot in ROTS and P >= 1 and 1 <= J <= 64
    rs = np.random.RandomState(seed)
    xyz = (rs.normal(0, 0.35, (P, 3)) * np.array([0.5, 1.0, 0.3])).astype(np.float32)

    def joints(r):
        A = np.tile(np.eye(4, dtype=np.float32), (J, 1, 1))
        for j in range(J):
            A[j, :3, :3] = lo.batch_rodrigues(torch.from_numpy(r.normal(0, 0.3, (1, 3)).astype(np.float32))).numpy()[0]
            A[j, :3, 3] = r.normal(0, 0.05, 3)
        return A
    A = joints(rs)
    w = rs.rand(P, J).astype(np.float32) ** 6
    w[w < 0.1] = 0
    perm = rs.permutation(J)
    w[np.arange(P), perm[np.arange(P) % J]] += 0.3
    w /= w.sum(1, keepdims=True)
    iso = rot == "iso"
    d6 = None if iso else rs.normal(size=(P, 6)).astype(np.float32)
    Rc = None if iso else lo.rotation_6d_to_matrix(torch.from_numpy(d6)).numpy()
    scales = (4.0 * np.exp(rs.normal(-4.6, 0.4, (P, 3)))).astype(np.float32)
    if iso:
        scales[:] = scales[:, :1]
    opac = rs.uniform(0.05, 0.95, (P, 1)).astype(np.float32)
    shs = np.concatenate([rs.normal(0, 1, (P, 1, 3)), rs.normal(0, 0.15, (P, 15, 3))], 1).astype(np.float32)
    transl = np.array([-0.04, 0.09, 4.0], np.float32)
    dL = rs.normal(0, 1, (3, H, W)).astype(np.float32)
    if K is not None:
        rk = np.random.RandomState(seed + 7919)
        A = np.stack([A] + [joints(rk) for _ in range(K - 1)])
        transl = np.stack([transl] + [(transl + rk.normal(0, 0.03, 3)).astype(np.float32) for _ in range(K - 1)])
        dL = np.stack([dL] + [rk.normal(0, 1, (3, H, W)).astype(np.float32) for _ in range(K - 1)])
    rot_in = None if iso else (d6 if rot == "6d" else Rc)
    return dict(N=P, P=P, J=J, K=K, W=W, H=H, rot=rot, xyz=xyz, A=A, w=w.astype(np.float32), d6=d6, Rc=Rc, rot_in=rot_in, scales=scales,
                opac=opac, shs=shs, cam=_camera(W, H), smpl_scale=np.array([1.07], np.float32), transl=transl,
                bg=np.array([1, 1, 1], np.float32), dL=dL)


def one_hot_joints(J, seed):
    """The joints a one-hot scene uses: 0 and J - 1, the first and the last joint of every 16-joint chunk when J > 16, and about
    half of the others -- at least one joint stays unused when J >= 3."""
    must = {0, J - 1}
    if J > 16:
        for c in range((J + 15) // 16):
            must |= {16 * c, min(16 * c + 15, J - 1)}
    others = [j for j in range(J) if j not in must]
    rs = np.random.RandomState(seed + 104729)
    rs.shuffle(others)
    keep = others[:len(others) // 2]                              # (len // 2 < len whenever there are others: one is left out)
    return sorted(must | set(keep))


def one_hot(P, J, seed, rot="6d"):
    """``scene`` with every weight row one-hot on one of ``one_hot_joints`` (``used``; Gaussian i on used[i % len(used)])."""
    s = scene(P, J, seed, rot)
    used = one_hot_joints(J, seed)
    assert P >= len(used)
    w = np.zeros((P, J), np.float32)
    w[np.arange(P), np.asarray(used)[np.arange(P) % len(used)]] = 1.0
    s["w"] = w
    s["used"] = used
    return s


# ---- the case lists ---------------------------------------------------------------------------------------------------------------
_SINGLE_PJ = ([(257, J) for J in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 42, 43, 47, 48, 49, 63, 64)]
              + [(P, J) for J in (17, 64) for P in (1, 63, 64, 65, 255, 256, 257, 300)])
_FRAMES_KPJ = ([(3, 257, J) for J in (1, 3, 16, 17, 42, 43, 49, 63, 64)] + [(2, P, J) for J in (17, 64) for P in (1, 63, 65, 256)]
               + [(16, 65, 64)])
# One seed per case, in list order: the smallest of base, base + 1000, base + 2000, ... (base = 100 / 200 / 300 / 400 + index) that
# meets every condition of tests/test_skin_edge_cases_host.py (the replacements: a Gaussian within 1e-3 of a matrix_to_quaternion
# branch change, a 6-D row so ill-conditioned that the fp32 restatement itself leaves a quarter of the GPU bar, and for P = 1 the
# lone Gaussian out of view).
_SINGLE_SEEDS = [2100, 101, 102, 2103, 104, 105, 1106, 107, 108, 1109, 110, 111, 5112, 113, 114, 3115, 116, 117, 118, 119, 120, 121, 122, 123,
                 1124, 125, 2126, 1127, 128, 129, 130, 1131, 132, 1133]
_FRAMES_SEEDS = [200, 1201, 202, 3203, 2204, 205, 3206, 1207, 208, 209, 210, 211, 7212, 213, 214, 215, 1216, 217]
_ONE_HOT_SEEDS = [300, 301, 302, 1303, 304]
_SCENE_SEEDS = [400, 401, 1402]
assert len(_SINGLE_SEEDS) == len(_SINGLE_PJ) and len(_FRAMES_SEEDS) == len(_FRAMES_KPJ)

# (P, J, seed, rot, SH degree): rot cycles through the three modes, degree 3 on odd indices and 0 on even ones
SINGLE = [(P, J, _SINGLE_SEEDS[i], ROTS[i % 3], 3 if i % 2 else 0) for i, (P, J) in enumerate(_SINGLE_PJ)]
# (K, P, J, seed, rot): SH degree 0, as the K-frame tests of tests/test_gpu_frames.py
FRAMES = [(K, P, J, _FRAMES_SEEDS[i], ROTS[i % 3]) for i, (K, P, J) in enumerate(_FRAMES_KPJ)]
# (P, J, seed): one-hot weight rows
ONE_HOT = [(65, J, _ONE_HOT_SEEDS[i]) for i, J in enumerate((1, 2, 17, 33, 64))]
# the scene forward's three avatars (P, J, seed, rot), K = 2
SCENE_K = 2
SCENE_AVATARS = [(P, J, _SCENE_SEEDS[i], rot) for i, (P, J, rot) in enumerate(((1, 1, "iso"), (65, 17, "6d"), (257, 64, "mat")))]


def case_id(c):
    return "-".join(str(v) for v in c)


def frame_of(s, f):
    """Frame f of a K-frame scene as a single-frame scene (shared arrays, not copies)."""
    if s["K"] is None:
        return s
    return dict(s, K=None, A=s["A"][f], transl=s["transl"][f], dL=s["dL"][f])


def all_frames():
    """Every (label, single-frame scene) the GPU file poses: SINGLE, every frame of FRAMES, ONE_HOT, the scene's avatars."""
    for c in SINGLE:
        yield "single-" + case_id(c), dict(scene(*c[:4]), deg=c[4], kind="single")
    for c in FRAMES:
        s = scene(c[1], c[2], c[3], c[4], K=c[0])
        for f in range(c[0]):
            yield f"frames-{case_id(c)}-f{f}", dict(frame_of(s, f), deg=0, kind="frames")
    for c in ONE_HOT:
        yield "one_hot-" + case_id(c), dict(one_hot(*c), deg=0, kind="one_hot")
    for c in SCENE_AVATARS:
        s = scene(c[0], c[1], c[2], c[3], K=SCENE_K)
        for f in range(SCENE_K):
            yield f"scene-{case_id(c)}-f{f}", dict(frame_of(s, f), deg=0, kind="scene")


# ---- the restatement on these scenes ----------------------------------------------------------------------------------------------
def deform(s, dtype=torch.float32, grad=False):
    """oracle/lbs_oracle.deform_gaussians on a single-frame scene in ``dtype`` -> (leaves, (xyz, q, scales, T)).  leaves: dict of
    ``xyz``, ``rot`` (the tensor in the form the kernels are handed: [P,6], [P,3,3] or None), ``scales``, ``A``, ``transl``."""
    T = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype).clone().requires_grad_(grad)
    lv = dict(xyz=T(s["xyz"]), rot=T(s["rot_in"]), scales=T(s["scales"]), A=T(s["A"]), transl=T(s["transl"]))
    if s["rot"] == "6d":
        Rc = lo.rotation_6d_to_matrix(lv["rot"])
    elif s["rot"] == "mat":
        Rc = lv["rot"]
    else:
        Rc = torch.eye(3, dtype=dtype)[None].repeat(s["P"], 1, 1)
    out = lo.deform_gaussians(lv["xyz"], Rc, lv["scales"], torch.from_numpy(s["w"]).to(dtype), lv["A"],
                              smpl_scale=torch.from_numpy(s["smpl_scale"]).to(dtype), transl=lv["transl"])
    return lv, out


def upstream(s, seed=5):
    """Random upstream gradients on the posed means [P,3], quaternions [P,4] and scales [P,3] (fp32 numpy)."""
    rs = np.random.RandomState(seed)
    return (rs.normal(size=(s["P"], 3)).astype(np.float32), rs.normal(size=(s["P"], 4)).astype(np.float32),
            rs.normal(size=(s["P"], 3)).astype(np.float32))


def lbs_gradients(s, gx, gq, gs, dtype=torch.float64):
    """dL/d(xyz_canon, rot_canon in the kernels' form, scales, A, transl) of <posed means, gx> + <quaternions, gq> + <scales, gs> by
    autograd through the restatement in ``dtype`` -> dict of float64 numpy arrays (``rot_canon`` None for isotropic scenes)."""
    lv, (x, q, sc, _) = deform(s, dtype, grad=True)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    loss = (x * t(gx)).sum() + (q * t(gq)).sum()
    if gs is not None:
        loss = loss + (sc * t(gs)).sum()
    loss.backward()
    g = lambda v: None if v is None else (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy().astype(np.float64))
    return dict(xyz_canon=g(lv["xyz"]), rot_canon=g(lv["rot"]), scales=g(lv["scales"]), A=g(lv["A"]), transl=g(lv["transl"]))


def bar_ratio(name, a, b, factor=1.0):
    """Largest |a - b| / (rtol |b| + atol max|b|) with BAR[name]'s pair times ``factor`` (tests/test_gpu_skinned._close's bound:
    <= 1 passes).  ``A`` compares rows [:, :3, :]."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if name == "A":
        a, b = a.reshape(-1, 4, 4)[:, :3, :], b.reshape(-1, 4, 4)[:, :3, :]
    rtol, atol = BAR[name]
    bound = factor * (rtol * np.abs(b) + atol * (np.abs(b).max() + 1e-30))
    return float((np.abs(a - b) / bound).max())
