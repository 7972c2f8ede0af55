"""The shapes of the size-threshold tests (tests/test_thresholds_cpu.py, tests/test_thresholds_gpu.py; DESIGN.md "Size
thresholds"): the limits at which a device path changes its algorithm, as constants, and the smallest inputs that cross
them.  Deterministic and vectorised: nothing here loops in Python over the items of a large shape.  TEST INFRASTRUCTURE
ONLY.

The rocPRIM numbers are those of the installed headers (rocprim/device/device_radix_sort.hpp: `size <=
single_sort_items_per_block`, then `size <= merge_sort_limit`, then onesweep; device_radix_sort_config.hpp and
detail/device_config_helper.hpp for the two values).  A test cannot see from Python which of the three ran: the shapes
keep to the limits as read there, and DESIGN.md's table is the record."""
import numpy as np

import multihit_oracle as mo
import nearest_cases as ncases
import signed_cases as scases
import signed_reference as sref

# ---- the limits ---------------------------------------------------------------------------------------------------------
SORT_SINGLE_BLOCK = 1024          # rocprim::radix_sort_pairs: up to this many items, one block sorts
SORT_MERGE_LIMIT = 1 << 20        # ... up to this many, block sort and merge; above it, onesweep
BUILD_LANES = 256                 # csrc/kernels/build.hip.h
INSTANCE_FUSED_PARTIALS = 256     # csrc/kernels/instance_build.hip.h: workgroups whose partials ride in the next kernel
INSTANCE_FUSED_LIMIT = INSTANCE_FUSED_PARTIALS * BUILD_LANES  # instances
INSTANCES_MAX = 1 << 20           # include/rt_hip_instances.h, RT_INSTANCES_MAX
VIEWS_SCAN = 1024                 # csrc/kernels/views.hip.h: sub-pixels per block of the hit list's counts ...
VIEWS_SUMS = 1024                 # ... and blocks per turn of views_scan_sums_kernel
VIEWS_TURN = VIEWS_SCAN * VIEWS_SUMS
VIEWS_MAX_CHUNK = 65535           # csrc/ray_query.cc
SIGNED_GRID_CHUNK = 1 << 24       # csrc/ray_query.cc: voxels per slab of the host form
BRICK = 4                         # csrc/kernels/signed.hip.h: a wave takes 4 x 4 x 4 voxels

# ---- A. instance sets -----------------------------------------------------------------------------------------------------
INSTANCE_COUNTS = (1024, 1025, 65536, 65537)  # astride the single-block sort, astride the fused reductions
INSTANCE_LARGEST = INSTANCES_MAX              # the largest set the library takes: still block sort and merge
INSTANCE_REFUSED = SORT_MERGE_LIMIT + 1       # the first onesweep size: more than RT_INSTANCES_MAX
RUN = 300                                     # identical transforms at the end of a set: longer than a workgroup
FIRST_GROUP = 5                               # an index in the first workgroup


def special_places(n: int) -> dict:
    """name -> index of the covering instance: in the first workgroup, in the last one, and at 65 536 where the set has it."""
    out = {"first": FIRST_GROUP, "last": n - 1}
    if n > INSTANCE_FUSED_LIMIT + 1:
        out["at_65536"] = INSTANCE_FUSED_LIMIT
    return out


def _rotations(rng, n: int) -> np.ndarray:
    """(n, 3, 3) proper rotations from unit quaternions."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def _about(A, centre, shift) -> np.ndarray:
    """(n, 3, 4): [A | t] that applies A about `centre` and then moves by `shift` (instance_cases._about, for many)."""
    W = np.zeros((len(A), 3, 4))
    W[:, :, :3] = A
    W[:, :, 3] = centre - A @ centre + shift
    return W


def instance_set(arrays, n: int, special_at: int, seed: int = 0):
    """(float32 (n, 3, 4), side): instance_cases.many's kind of set without its loop -- translated, rotated and scaled copies
    scattered over a cube of `side` that grows with n --, its last RUN transforms one and the same (equal keys across a
    256-lane workgroup; the tie goes by instance index), and at `special_at` ONE copy large enough to cover the cube: it
    alone touches all six faces of the tree's root box, and -- a copy that covers the others reaches further than they --
    its reach is the set's largest.  A reduction that drops the partial of its workgroup changes G = 4 x reach and with it
    every leaf box, and the root box and with it every key."""
    assert n >= RUN + 2 and 0 <= special_at < n
    lo, hi = mo.box_of(arrays)
    centre, ext = (lo + hi) / 2, hi - lo
    rng = np.random.default_rng(7000 + n + seed)
    side = float(n) ** (1.0 / 3.0) * ext.max() * 1.5
    A = _rotations(rng, n) * rng.uniform(0.5, 1.5, n)[:, None, None]
    W = _about(A, centre, (rng.random((n, 3)) - 0.5) * side)
    W[n - RUN:] = W[n - RUN]
    # every copy lies within side / 2 + 1.5 * |ext| of the centre on every axis; the cover's half-size is cover * ext / 2
    cover = 2.0 * (side / 2 + 1.5 * float(np.linalg.norm(ext))) / float(ext.min()) * 1.25
    W[special_at] = _about(np.eye(3)[None] * cover, centre, np.zeros(3))[0]
    return np.ascontiguousarray(W, np.float32), side


def reaches(arrays, W) -> np.ndarray:
    """(n,) float64: the reach of every instance (instance_cases.set_reach before its maximum)."""
    lo, hi = mo.box_of(arrays)
    absW = np.abs(np.asarray(W, np.float64))
    return (absW[:, :, :3] @ np.maximum(np.abs(lo), np.abs(hi)) + absW[:, :, 3]).max(axis=1)


def face_touchers(nodes, n: int) -> np.ndarray:
    """(6, n) bool: which instances' leaf boxes attain the root box of the tree on lo x, y, z, hi x, y, z."""
    leaves = nodes[nodes["leaf"] != 0xFFFFFFFF]
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    lo[leaves["leaf"]], hi[leaves["leaf"]] = leaves["lo"], leaves["hi"]
    return np.concatenate([(lo == nodes["lo"][0]).T, (hi == nodes["hi"][0]).T])


def groups_of(n: int) -> int:
    return (n + BUILD_LANES - 1) // BUILD_LANES


# ---- B. a scene past the merge limit --------------------------------------------------------------------------------------
TERRAIN = 725            # tools.big_meshes.terrain(725): 1 051 250 faces, the first terrain above SORT_MERGE_LIMIT
TERRAIN_FACES = 2 * TERRAIN * TERRAIN
TERRAIN_RESTATED = 200   # ... and the size at which the CPU file holds build_lbvh against the numpy restatement
TERRAIN_COPIES = 70      # copies of one face behind the field: the field's own equal keys come in pairs at the most
TERRAIN_COPIED = 333333  # ... of this face


def big_terrain():
    """(vertices (V, 3), faces (TERRAIN_FACES + TERRAIN_COPIES, 3)): the field, then TERRAIN_COPIES copies of one of its faces
    -- a run of equal keys that must come out in rising face id."""
    from tools.big_meshes import terrain

    v, f = terrain(TERRAIN)
    assert len(f) == TERRAIN_FACES
    return v, np.ascontiguousarray(np.concatenate([f, np.repeat(f[TERRAIN_COPIED:TERRAIN_COPIED + 1], TERRAIN_COPIES, axis=0)]))


def longest_run(sorted_keys) -> int:
    """The length of the longest run of equal values in a sorted array."""
    k = np.asarray(sorted_keys)
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    return int(np.diff(np.concatenate([starts, [len(k)]])).max())


def terrain_rays(vertices, n: int, seed: int):
    """(origins, directions) float32 (n, 4): from above the field down into it, a third x 37, a third x 0.01; every tenth
    from inside the field's box in a random direction."""
    rng = np.random.default_rng(seed)
    lo, hi = ncases.box_of(vertices)
    o = np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), np.full(n, hi[2] + 0.5)], axis=1)
    target = np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), np.full(n, lo[2])], axis=1)
    d = target - o
    inside = np.arange(n) % 10 == 9
    o[inside] = lo + rng.random((int(inside.sum()), 3)) * (hi - lo)
    d[inside] = rng.normal(size=(int(inside.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.array([1.0, 37.0, 0.01])[np.arange(n) % 3][:, None]
    out_o, out_d = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    out_o[:, :3], out_d[:, :3] = o, d
    return out_o, out_d


# ---- C. the sign table ----------------------------------------------------------------------------------------------------
BOOK_PAGES = 300
SIGN_POINT_SEED = 11  # (tests/test_thresholds_cpu.py: the float64 reference judges all but 1 % of these points)


def book(pages: int = BOOK_PAGES):
    """(vertices (pages + 2, 3), faces (pages, 3)): `pages` triangles around ONE shared edge, a non-manifold fan.  The edge
    (0, 1) is used by every face and both its vertices lie in every face: one edge segment and two vertex segments of
    `pages` members each in the sign table's sorts.  The pages differ in angle, width and height, so that no two corner
    angles or normals are equal and a sum taken in another order shows in its last bits."""
    k = np.arange(pages)
    angle = 2.0 * np.pi * (k + 0.37 * np.sin(k * 1.3)) / pages
    width = 0.6 + 0.4 * np.cos(k * 0.7) ** 2
    outer = np.stack([width * np.cos(angle), width * np.sin(angle), 0.5 + 0.45 * np.sin(k * 2.1)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], outer])
    f = np.stack([np.zeros(pages), np.ones(pages), k + 2], axis=1)
    return v.astype(np.float32), f.astype(np.uint32)


def sign_meshes() -> dict:
    """name -> (maker, closed, points of the signed queries, with per-feature points)."""
    return {
        "torus_600x300": (lambda: scases.torus(around=600, across=300), True, 256, False),  # 1 080 000 corners: onesweep, both widths
        "torus_24x14": (lambda: scases.torus(around=24, across=14), True, 512, True),       # 2 016 corners: past one block
        "star": (lambda: scases.star(), True, 512, True),                                   # 84 corners: one block
        "star_200": (lambda: scases.star(points=200), True, 512, True),                     # apexes of valence 400
        "book": (book, False, 512, True),                                                   # one edge of 300 faces
    }


def segment_lengths(faces):
    """(the most corners at one vertex, the most faces at one edge)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valence = np.bincount(f.reshape(-1)).max()
    pairs = np.sort(np.concatenate([f[:, [0, 1]], f[:, [0, 2]], f[:, [1, 2]]]), axis=1)
    uses = np.unique(pairs[:, 0] * (int(f.max()) + 1) + pairs[:, 1], return_counts=True)[1].max()
    return int(valence), int(uses)


def signed_points(vertices, faces, total: int, seed: int, features: bool):
    """(points float32 (total, 3), judged bool (total,)): points in the mesh's box x 1.5, far away, displaced from features
    along their pseudonormals (`features`; a Python loop over the mesh: small meshes only), ON the surface, and the odd
    ones.  `judged`: the points tests/signed_reference.py speaks about -- finite and off the surface by construction."""
    odd = ncases.odd_points(vertices)
    surface = total // 8
    feature = total // 5 if features else 0
    far = total // 12
    box = total - len(odd) - surface - feature - far
    parts = [ncases.in_box(vertices, box, seed), ncases.far_away(vertices, far, seed + 2)]
    if feature:
        every = scases.per_feature(vertices, faces)[0]
        parts.append(every[np.linspace(0, len(every) - 1, feature).astype(np.int64)])
    judged = sum(len(p) for p in parts)
    parts += [ncases.on_surface(vertices, faces, surface, seed + 1), odd]
    points = np.ascontiguousarray(np.concatenate(parts), np.float32)[:, :3]
    assert len(points) == total, (len(points), total)
    return points, np.arange(total) < judged


class _OnDemand(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        self[key] = self.make(key)
        return self[key]


class LazyPseudonormals(sref.Pseudonormals):
    """signed_reference.Pseudonormals for a mesh of a million corners: the face normals at once, a vertex's or an edge's sum
    when of_nearest asks for it -- over the faces at that vertex in file order, term for term the sum the base class
    makes in its loop over all faces (tests/test_thresholds_cpu.py holds the two against each other on a small torus)."""

    def __init__(self, vertices, faces):
        self.v = np.asarray(vertices, np.float64)[:, :3]
        self.f = np.asarray(faces, np.int64).reshape(-1, 3)
        tri = self.v[self.f]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        self.length = np.linalg.norm(n, axis=1)
        self.face = np.where(self.length[:, None] > 0.0, n / np.where(self.length > 0.0, self.length, 1.0)[:, None], 0.0)
        corners = self.f.reshape(-1)
        self.order = np.argsort(corners, kind="stable")  # (corner 3 k + c of face k: a vertex's corners in rising face)
        self.start = np.searchsorted(corners[self.order], np.arange(len(self.v) + 1))
        self.vertex, self.edge = _OnDemand(self.vertex_sum), _OnDemand(self.edge_sum)

    def corners_at(self, x: int):
        for at in self.order[self.start[x]:self.start[x + 1]]:
            yield divmod(int(at), 3)

    def vertex_sum(self, x: int) -> np.ndarray:
        total = np.zeros(3)
        for k, corner in self.corners_at(x):
            ids = self.f[k]
            y, z = int(ids[(corner + 1) % 3]), int(ids[(corner + 2) % 3])
            w = sref.angle64(self.v[y] - self.v[x], self.v[z] - self.v[x]) if self.length[k] > 0.0 else 0.0
            total = total + w * self.face[k]
        return total

    def edge_sum(self, key) -> np.ndarray:
        total, seen = np.zeros(3), set()
        for k, _ in self.corners_at(key[0]):
            if k in seen:
                continue
            seen.add(k)
            ids = [int(i) for i in self.f[k]]
            for corner in range(3):
                x, y = ids[corner], ids[(corner + 1) % 3]
                if (min(x, y), max(x, y)) == key:
                    total = total + self.face[k]
        return total


def compare_in_batches(points, vertices, faces, inside, closed: bool, batch: int, normals=None, threads: int = 8) -> dict:
    """signed_reference.compare over batches of `batch` points -- its float64 arrays are points x faces --, side by side on
    `threads` threads (numpy's array operations run without the interpreter's lock), its cap on the excluded share applied
    to the whole set instead of to each batch."""
    from concurrent.futures import ThreadPoolExecutor

    violations, judged = [], 0
    firsts = list(range(0, len(points), batch))
    with ThreadPoolExecutor(max_workers=threads) as pool:
        results = list(pool.map(lambda first: sref.compare(points[first:first + batch], vertices, faces, inside[first:first + batch], closed,
                                                           normals=normals), firsts))
    for first, held in zip(firsts, results):
        violations += [f"[{first}..] {text}" for text in held["violations"] if "lies within the distance tolerance" not in text]
        judged += held["judged"]
    excluded = 1.0 - judged / max(1, len(points))
    if excluded > sref.EXCLUDED_CAP:
        violations.append(f"{excluded:.4f} of the set lies within the distance tolerance of the surface (cap {sref.EXCLUDED_CAP})")
    return {"violations": violations, "excluded": excluded, "judged": judged}


# ---- D. the grid's slabs --------------------------------------------------------------------------------------------------
GRID_SEAM = (1024, 1639, 11)                          # a slice of 1 678 336 voxels: slabs of 9 and 2 slices
GRID_THIN = (4, 4, SIGNED_GRID_CHUNK // 16 + 3)       # a slice of 16: slabs of 2^20 and 3 slices
GRID_WIDE = (4097, 4097, 2)                           # a slice larger than a slab: one slice a slab


def slabs(dims) -> list:
    """[(first slice, slices)] of RayQueries::signedGridHost, restated."""
    slice_ = dims[0] * dims[1]
    per_slab = min(dims[2], max(1, SIGNED_GRID_CHUNK // slice_))
    return [(first, min(per_slab, dims[2] - first)) for first in range(0, dims[2], per_slab)]


def grid_over(vertices, dims, factor: float = 1.25):
    """(origin, spacing) float32 (3,): the grid of `dims` voxels over the mesh's box x factor."""
    lo, hi = ncases.box_of(vertices)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * factor
    origin = (centre - half).astype(np.float32)
    spacing = (2 * half / np.maximum(1, np.asarray(dims, np.float64) - 1)).astype(np.float32)
    return origin, spacing


def is_power_of_two(x) -> bool:
    m, _ = np.frexp(np.float32(x))
    return bool(m == 0.5)


# ---- E. the hit list and the views chunk ----------------------------------------------------------------------------------
ONE_VIEW = dict(width=1100, height=960, n_super_samples=1)   # 1 056 000 sub-pixels: 1 032 blocks
MANY_VIEWS = dict(width=37, height=23, n_super_samples=16)   # 4 x 4 a pixel: 13 616 sub-pixels a view ...
MANY_VIEWS_COUNT = 78                                        # ... 1 062 048 in one chunk
TINY_VIEW = dict(width=2, height=2, n_super_samples=1)
TINY_VIEWS_COUNT = VIEWS_MAX_CHUNK + 2                       # 65 537 views: two chunks
TINY_VIEWS_CHECKED = 64
TINY_RADIUS = 2.0 / 16.0
MANY_VIEWS_AWAY = 75                                         # the view that sees nothing: blocks 997 .. 1 010 are empty


def close_pose(rt):
    """orbit_135 of the blob at 1 / 16 of its size from half the distance: the mesh fills the image."""
    a = np.radians(135)
    return rt.Camera.look_at((np.sin(a) / 16, 0.15 / 16, np.cos(a) / 16), (0, 0, 0))


def orbit_poses(rt, count: int, away: int) -> list:
    """`count` poses above the blob at 1 / 16 of its size -- a slab of 6 x 1.27 x 6, its top at y = 0.64 --, looking down at
    its centre from changing heights and sides; view `away` looks up, out of the scene."""
    out = []
    for k in range(count):
        a = 2.0 * np.pi * k / count
        eye = np.array([1.2 * np.sin(a), 1.2 + 0.4 * np.sin(3.0 * a + 0.4), 1.2 * np.cos(a)]) / 16.0
        out.append(rt.Camera.look_at(tuple(eye), tuple(2.0 * eye) if k == away else (0.0, 0.0, 0.0)))
    return out


def sub_pixels(size: dict, views: int = 1) -> int:
    """(n_super_samples counts the samples of a pixel: a grid of its square root a side)"""
    grid = int(round(size["n_super_samples"] ** 0.5))
    assert grid * grid == size["n_super_samples"]
    return views * size["width"] * size["height"] * grid * grid


def scan_blocks(size: dict, views: int = 1) -> int:
    return (sub_pixels(size, views) + VIEWS_SCAN - 1) // VIEWS_SCAN


def tiny_poses(count: int, radius: float, seed: int = 3) -> np.ndarray:
    """float32 (count, 4, 3) -- eye, right, up, forward, the twelve floats a views call uses as given and the oracle takes
    too --: eyes on a sphere of `radius` around the origin, looking at it; every seventh looks away."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(count, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    eye = e * radius
    forward = np.where((np.arange(count) % 7 == 6)[:, None], e, -e)
    helper = np.where((np.abs(forward[:, 1]) < 0.9)[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
    right = np.cross(forward, helper)
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    return np.ascontiguousarray(np.stack([eye, right, np.cross(right, forward), forward], axis=1), np.float32)


def checked_views(count: int = TINY_VIEWS_COUNT, checked: int = TINY_VIEWS_CHECKED) -> np.ndarray:
    """`checked` view indices spread over both chunks, the last of the first chunk and the first of the second among them."""
    spread = np.linspace(0, count - 1, checked - 3).astype(np.int64)
    out = np.unique(np.concatenate([spread, [VIEWS_MAX_CHUNK - 1, VIEWS_MAX_CHUNK, VIEWS_MAX_CHUNK + 1]]))
    extra = [v for v in (1, 2, 3, VIEWS_MAX_CHUNK - 2) if v not in out]
    return np.sort(np.concatenate([out, extra[:checked - len(out)]])).astype(np.int64)
