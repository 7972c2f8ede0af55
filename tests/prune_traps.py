"""Frames in which a wrong growth of the leaves' boxes changes pixels (scene_pack.h, leaf_growth; kernels/primary.hip.h,
far_limit) -- a generator, no stored files.  Each scene is built FROM THE CAMERA'S OWN RAYS.

Image 64 x 8, one sample, focal length 50: every ray lies within 1e-2 rad of the camera's forward axis.  In the camera's
own coordinates (the reference camera's: eye (0, 0, 2), looking along -z), per pixel column, outermost first (j = 0) on
each side s = +-1 of the centre:
  * a front triangle Y in the plane  s x + z = 1 - 0.01 j  with edges u = S (s, 0, -1) and v = (0, 0.2, 0), placed so that
    the column's ray crosses its plane at the parameters (-0.5e-5, ~0.5): OUTSIDE the triangle, inside the slack of the
    reference's test, which accepts the hit -- and outside Y's own box in x by 0.5e-5 S: the ray enters that box only
    0.5e-5 S / |px| later;
  * a thin back triangle X centred on the same ray halfway along that stretch, across it, narrower than the pixel pitch,
    spanning all rows -- and leaning towards the eye by 0.05 per unit of height, 0.6 high: its box begins in front of Y's
    (the walk lists children nearest to the eye first; with X upright Y is always met first, and a lane that holds Y's hit
    has nothing left to lose -- a sequential model of the walk showed no pixel of (a) changing without the growth).
A pixel is a TRAP when its winning hit lies in front of its leaf's own box, another accepted hit lies behind it, and the
own box's near distance exceeds that hit's d (1 + 1e-5) + prune_margin: with un-grown boxes a lane that holds the other
hit would not enter the winner's box.  (tests/prune_bound_sweep.cc, `facts`, computes that from the reference's float
triangle test and double box distances alone.)

Placements: "a" the reference's camera; "b" the same construction with the axes permuted, seen by a posed camera on +x
looking along -x; "c" scene and eye translated together by the dyadic offset (64, -32, 16), the front triangles 16 times as
long so that the slack strip is 16 ulps of the coordinates and more, and only the columns kept whose entry stretch is four
times prune_margin or more.

ties_mesh(ordinary_first): a face without a bound (a needle, eta = 1/8) and an ordinary face in the plane z = 0 with dyadic coordinates
and power-of-two normals -- a ray through both gets bit-equal distances, and the closest hit is the LOWER LEAF, whichever
side of the unpruned head of the walk records that leaf lies on.  `ordinary_first` swaps the two leaves' order.  The needle
shares a vertex with a tilted face out of view, so its smooth normal differs from the ordinary face's: the pixel shows who won.
"""
import os
import subprocess

import numpy as np

import orc
import query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEIGHT, FOCAL = 64, 8, 50.0

POSES = {
    "a": np.array([[0, 0, 2], [1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32),
    "b": np.array([[2, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0]], np.float32),
    "c": np.array([[64, -32, 18], [1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32),
}
SCALE = {"a": 1.0, "b": 1.0, "c": 16.0}
LEAN = 0.05


def options(rt, **more):
    return rt.Options.defaults(width=WIDTH, height=HEIGHT, n_super_samples=1, focal_length=FOCAL, ao_num_samples=2, **more)


def posed_rays(params, pose):
    """The posed camera's rays as tests/camera_oracle.c makes them, float operation for float operation:
    w = ((right cx) + (up cy)) + forward, direction = w / sqrt((wx wx + wy wy) + wz wz)."""
    f = np.float32
    W, H = int(params.width), int(params.height)
    a = f(params.focal_length) * f(max(W, H))
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    cx = ((x + f(0.5)) / a - f(W) / (f(2.0) * a)).reshape(-1)
    cy = (-((y + f(0.5)) / a - f(H) / (f(2.0) * a))).reshape(-1)
    pose = np.asarray(pose, np.float32)
    w = [((pose[1, k] * cx) + (pose[2, k] * cy)) + pose[3, k] for k in range(3)]
    length = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    o4, d4 = np.zeros((W * H, 4), np.float32), np.zeros((W * H, 4), np.float32)
    o4[:, :3] = pose[0]
    for k in range(3):
        d4[:, k] = w[k] / length
    return o4, d4


def rays(rt, placement):
    params = orc.params_from_options(options(rt))
    if placement == "a":
        return qo.camera_rays(params)
    return posed_rays(params, POSES[placement])


def trap_mesh(rt, placement):
    """(vertices float32 (n, 3), faces uint32 (m, 3), kind per face: ("Y" | "X", column))."""
    pose = POSES[placement].astype(np.float64)
    eye, right, up, back = pose[0], pose[1], pose[2], -pose[3]
    scale = SCALE[placement]
    _, d4 = rays(rt, placement)
    d = d4[:, :3].astype(np.float64).reshape(HEIGHT, WIDTH, 3)[HEIGHT // 2]
    # what prune_margin will be, roughly: 1e-5 of the largest magnitude among the eye's distance and the boxes' coordinates
    margin = 1e-5 * (np.abs(eye).max() + 3.0 + 1.5 * scale)
    verts, faces, kinds = [], [], []

    def world(p):  # camera coordinates (the reference camera's: the eye at (0, 0, 2)) -> the placement's
        p = np.asarray(p, np.float64)
        return eye + right * p[0] + up * p[1] + back * (p[2] - 2.0)

    def add(kind, column, a, b, c):
        base = len(verts)
        verts.extend([world(a), world(b), world(c)])
        faces.append((base, base + 1, base + 2))
        kinds.append((kind, column))

    for column in range(WIDTH):
        px = (d[column] @ right) / -(d[column] @ back)  # the ray is (mu px, ., 2 - mu) in the camera's coordinates
        side = 1.0 if px > 0 else -1.0
        j = WIDTH - 1 - column if px > 0 else column
        mu = (1.0 + 0.01 * j) / (1.0 - side * px)
        stretch = 0.5e-5 * scale / abs(px)
        if stretch < 4.0 * margin:
            continue
        u, v = scale * np.array([side, 0.0, -1.0]), np.array([0.0, 0.2, 0.0])
        at = np.array([mu * px, 0.0, 2.0 - mu]) + 0.5e-5 * u - 0.5 * v
        add("Y", column, at, at + u, at + v)
        mid = mu + 0.5 * stretch
        centre = np.array([mid * px, 0.0, 2.0 - mid])
        across = np.array([1.0, 0.0, px]) / np.hypot(1.0, px)
        # (it leans towards the eye -- LEAN along the ray per unit of height --, so that its box begins in FRONT of Y's: the
        # walk lists children nearest first, and a lane prunes Y's box only if it has met X before)
        along = np.array([0.0, 1.0, 0.0]) + LEAN * np.array([-px, 0.0, 1.0]) / np.hypot(1.0, px)
        half, below, above = 1.25e-4, 4.0e-3, 0.6
        add("X", column, centre - half * across - below * along, centre + half * across - below * along, centre + above * along)
    return np.array(verts, np.float64).astype(np.float32), np.array(faces, np.uint32), kinds


def ties_mesh(ordinary_first):
    """(vertices, faces, names): the needle N, the ordinary face O in its plane, the tilted face T that shares N's vertex
    b, and a quad behind them.  Every coordinate is dyadic; N's normal is (0, 0, 2^-3), O's (0, 0, 16).  `ordinary_first`
    turns O about the origin, which puts its leaf before N's."""
    y0 = -(2.0 ** -6)
    verts = [(-2, y0, 0), (2, y0, 0), (2, y0 + 2.0 ** -5, 0)]  # N: height 0 at x = -2 to 2^-5 at x = 2: y in [-2^-6, 0] at x = 0
    verts += [(1, 1, 0), (-3, 1, 0), (1, -3, 0)] if ordinary_first else [(-1, -1, 0), (3, -1, 0), (-1, 3, 0)]  # O
    verts += [(3, -1, -1), (3, 1, -1),                              # T = (N's b, these two): out of view
              (-4, -4, -1), (4, -4, -1), (4, 4, -1), (-4, 4, -1)]   # the quad behind
    faces = [(0, 1, 2), (3, 4, 5), (1, 6, 7), (8, 9, 10), (8, 10, 11)]
    return np.array(verts, np.float32), np.array(faces, np.uint32), ["N", "O", "T", "B", "B"]


def product_scene(rt, vertices, faces):
    """(product Scene with its BVH, SceneArrays for the oracles)."""
    scene = rt.Scene.from_arrays(vertices, faces).build_bvh(0)
    return scene, orc.SceneArrays.from_scene(scene)


_EXE = {}


def sweep_program(tmp_dir, lib="lib"):
    """tests/prune_bound_sweep.cc, compiled once per session against the product library (`lib_knobs`: the A/B build)."""
    if lib not in _EXE:
        exe = os.path.join(str(tmp_dir), "prune_bound_sweep_" + lib)
        lib_dir = os.path.join(ROOT, "opencl_raytracer_amd", lib)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "opencl_raytracer_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "prune_bound_sweep.cc"), "-L" + lib_dir, "-locrt_hip",
                        "-Wl,-rpath," + lib_dir], check=True)
        _EXE[lib] = exe
    return _EXE[lib]


def write_scene(tmp_dir, name, vertices, faces, o4, d4):
    """(scene.off, rays.f32) for tests/prune_bound_sweep.cc."""
    off, ray_file = (os.path.join(str(tmp_dir), name + ext) for ext in (".off", ".rays"))
    with open(off, "w") as f:
        f.write("OFF\n%d %d 0\n" % (len(vertices), len(faces)))
        for v in vertices:
            f.write("%.9g %.9g %.9g\n" % tuple(float(x) for x in v[:3]))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(x) for x in t))
    np.concatenate([qo.as4(o4), qo.as4(d4)], axis=1).astype(np.float32).tofile(ray_file)
    return off, ray_file


def facts(exe, tmp_dir, name, vertices, faces, o4, d4):
    """What tests/prune_bound_sweep.cc `facts` says about the scene and the rays, from the reference's tests alone:
    {"prune_margin", "unpruned_bytes", "primary_bytes", "covered", "face" (per leaf), "growth", "loose", "eta",
     "winner" (leaf per ray, -1: none), "in_front", "trap" (per ray), "accepted" (per ray: [(leaf, distance word)])}."""
    off, ray_file = write_scene(tmp_dir, name, vertices, faces, o4, d4)
    out = os.path.join(str(tmp_dir), name + ".facts")
    subprocess.run([exe, "facts", off, ray_file, out], check=True)
    n = len(o4)
    r = {"face": [], "growth": [], "loose": [], "eta": [], "winner": np.full(n, -1), "in_front": np.zeros(n, bool),
         "trap": np.zeros(n, bool), "accepted": [None] * n}
    with open(out) as f:
        for line in f:
            w = line.split()
            if w[0] == "facts":
                r.update(prune_margin=float.fromhex(w[1]), unpruned_bytes=int(w[2]), primary_bytes=int(w[3]), covered=bool(int(w[4])))
            elif w[0] == "leaf":
                assert int(w[1]) == len(r["face"])
                r["face"].append(int(w[2]))
                r["growth"].append(float.fromhex(w[3]))
                r["loose"].append(bool(int(w[4])))
                r["eta"].append(float.fromhex(w[5]))
            elif w[0] == "ray":
                i = int(w[1])
                r["winner"][i], r["in_front"][i], r["trap"][i] = int(w[2]), bool(int(w[3])), bool(int(w[4]))
                r["accepted"][i] = [(int(w[6 + 2 * k]), int(w[7 + 2 * k])) for k in range(int(w[5]))]
    return r
