"""Mesh fixtures for the rasteriser tests (test_shot_item_cpu.py, test_gpu_shot_item.py): deterministic, seeded, numpy only.

irbpp_shot_item_kernel stages the faces through LDS in chunks of CHUNK = 128 and casts RAYS_PER_GROUP = 256 rays per workgroup;
the builders here hit face counts exactly, put the faces a ray can cross into chosen chunks, spread rays over more than one
workgroup, and keep slanted solids in generic position (no ray on the projection of an edge), so that "inside" has one answer.
``exact_tables`` evaluates the inside test and the plane height of oracle/shot.py with fractions.Fraction on the float64
coordinates: the yardstick the (trimesh-unpinned) oracle itself is held to on the CPU.
"""
from fractions import Fraction
from functools import lru_cache

import numpy as np

from irbpp_amd import meshes
from oracle.shot import shot_item

CHUNK = 128                 # SHOT_CHUNK of csrc/irbpp_kernels.hip
RAYS_PER_GROUP = 256        # rays (threads) of one workgroup of irbpp_shot_item_kernel


def at_origin(verts):
    """Bounding-box minimum at the origin, as tools.shot_item leaves the mesh (tools.py:100) and oracle.shot expects it."""
    verts = np.asarray(verts, dtype=np.float64)
    return verts - verts.min(0)


def grid(verts, res_h):
    """(fx, fy) of the ray grid, by the oracle's own expression."""
    ext = at_origin(verts).max(0)
    fx, fy = np.ceil(np.round(ext[0:2], decimals=6) / res_h).astype(np.int32)
    return int(fx), int(fy)


def areas(verts, faces):
    """Signed doubled xy-area of every face, in the oracle's expression (0.0 exactly: edge-on)."""
    a, b, d = (verts[faces[:, k]] for k in range(3))
    return (b[:, 0] - a[:, 0]) * (d[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (d[:, 0] - a[:, 0])


# ------------------------------------------------------------------ builders ------------------------------------------------
def voxel_solid(seed=5, dims=(4, 4, 3), cube=0.02, fill=0.5):
    """meshes.voxel_mesh of a random occupancy (every exposed voxel face two triangles): several hundred faces, all of them
    flat or edge-on; opposite corners occupied so that the extents are the full dims * cube."""
    rng = np.random.RandomState(seed)
    occ = rng.rand(*dims) < fill
    occ[0, 0, 0] = occ[-1, -1, -1] = True
    verts, faces = meshes.voxel_mesh(occ, cube)
    return verts, faces, occ


def height_field(n, m, ex, ey, seed=3, zlo=0.02, zhi=0.06):
    """A closed solid under a jittered n x m grid of vertices with random z: 2(n-1)(m-1) slanted top faces, two flat bottom
    faces, 4(n-1 + m-1) vertical side faces.  Interior vertices move by up to 0.3 grid spacings in x and y, border vertices
    along the border only, the corners stay: the footprint is the rectangle [0, ex] x [0, ey]."""
    rng = np.random.RandomState(seed)
    hx, hy = ex / (n - 1), ey / (m - 1)
    x = np.repeat(np.linspace(0.0, ex, n)[:, None], m, axis=1) + rng.uniform(-0.3, 0.3, size=(n, m)) * hx
    y = np.repeat(np.linspace(0.0, ey, m)[None, :], n, axis=0) + rng.uniform(-0.3, 0.3, size=(n, m)) * hy
    x[0, :], x[-1, :], y[:, 0], y[:, -1] = 0.0, ex, 0.0, ey
    y[0, 0], y[-1, 0], y[0, -1], y[-1, -1] = 0.0, 0.0, ey, ey
    x[0, 0], x[0, -1], x[-1, 0], x[-1, -1] = 0.0, 0.0, ex, ex
    z = rng.uniform(zlo, zhi, size=(n, m))
    top = np.stack([x, y, z], axis=2).reshape(n * m, 3)
    vid = lambda i, j: i * m + j                                                 # noqa: E731
    faces = []
    for i in range(n - 1):
        for j in range(m - 1):
            faces += [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)]]
    foot = top.copy()
    foot[:, 2] = 0.0                                                             # the border's shadow on z = 0
    low = lambda i, j: n * m + vid(i, j)                                         # noqa: E731
    faces += [[low(0, 0), low(n - 1, m - 1), low(n - 1, 0)], [low(0, 0), low(0, m - 1), low(n - 1, m - 1)]]
    border = ([(i, 0) for i in range(n)] + [(n - 1, j) for j in range(1, m)] + [(i, m - 1) for i in range(n - 2, -1, -1)] +
              [(0, j) for j in range(m - 2, -1, -1)])
    for (i0, j0), (i1, j1) in zip(border[:-1], border[1:]):
        faces += [[vid(i0, j0), low(i1, j1), vid(i1, j1)], [vid(i0, j0), low(i0, j0), low(i1, j1)]]
    return np.vstack([top, foot]), np.asarray(faces, dtype=np.int32)


def single_triangle():
    """One slanted face: the smallest mesh the entry point accepts."""
    return np.array([[0.0, 0.0, 0.01], [0.047, 0.004, 0.03], [0.011, 0.038, 0.0]]), np.array([[0, 1, 2]], dtype=np.int32)


def edge_on_faces(verts, count, seed=0):
    """`count` zero-area vertical triangles on existing vertices (a, a lifted, b): two corners share x and y, so the oracle's
    area expression is X*Y - Y*X = 0.0 exactly, in any pose about z.  Returns (verts with the lifted copies, new faces)."""
    rng = np.random.RandomState(seed)
    nv = len(verts)
    zmax = verts[:, 2].max()
    a = rng.randint(0, nv, size=count)
    b = (a + 1 + rng.randint(0, nv - 1, size=count)) % nv
    lifted = verts[a].copy()
    lifted[:, 2] = 0.5 * (lifted[:, 2] + zmax)                                  # inside [0, zmax]: the extents stay
    new = np.stack([a, nv + np.arange(count), b], axis=1).astype(np.int32)
    return np.vstack([verts, lifted]), new


def pad_to(verts, faces, count, seed=0, kind="both"):
    """The mesh with exactly `count` faces: edge-on triangles and duplicates of existing faces appended alternately
    (kind "edge_on": only the former).  Neither changes a table: an edge-on face is never crossed, a duplicate repeats a height."""
    extra = count - len(faces)
    assert extra >= 0
    n_edge = extra if kind == "edge_on" else (extra + 1) // 2
    v2, edge = edge_on_faces(verts, n_edge, seed)
    dup = faces[np.arange(extra - n_edge) % len(faces)]
    tail = np.empty((extra, 3), dtype=np.int32)
    if kind == "edge_on":
        tail[:] = edge
    else:
        tail[0::2], tail[1::2] = edge, dup
    return v2, np.vstack([faces, tail]).astype(np.int32)


def permuted(faces, seed=0):
    return faces[np.random.RandomState(seed).permutation(len(faces))]


def last_chunk_only(verts, faces, count=300):
    """`count` faces of which every one a ray can cross sits in the LAST chunk of CHUNK: the vertical sides and edge-on
    padding in front, top and bottom faces at the very end."""
    ar = areas(verts, faces)
    hit, side = faces[ar != 0.0], faces[ar == 0.0]
    assert len(hit) <= count - CHUNK * ((count - 1) // CHUNK)
    v2, pad = edge_on_faces(verts, count - len(faces), seed=1)
    return v2, np.vstack([side, pad, hit]).astype(np.int32)


def edge_on_middle_chunk(verts, faces, count=300):
    """`count` faces (three chunks) whose middle chunk [CHUNK, 2*CHUNK) is entirely edge-on, with faces a ray can cross in
    the chunks on both sides of it."""
    ar = areas(verts, faces)
    hit, side = faces[ar != 0.0], faces[ar == 0.0]
    v2, pad = edge_on_faces(verts, count - len(faces), seed=2)
    edge = np.vstack([side, pad])
    h0 = hit[:len(hit) // 2]
    first = np.vstack([h0, edge[:CHUNK - len(h0)]])
    rest = edge[CHUNK - len(h0):]
    out = np.vstack([first, rest[:CHUNK], hit[len(hit) // 2:], rest[CHUNK:]]).astype(np.int32)
    assert len(out) == count
    return v2, out


PICKET_BARS, PICKET_WIDTH, PICKET_LEN, PICKET_Z = 17, 0.0004, 0.165, 0.03


def picket(with_plate=False):
    """Bars PICKET_WIDTH wide at x = k * 0.01, along y: at res_h = 0.01 the rays pass at k * 0.01 + 0.001, between them, so
    nothing is hit over a 17 x 17 footprint (two workgroups, two chunks).  `with_plate`: plus one horizontal plate at
    z = 0.01 around the ray (16, 8) alone, which belongs to the last workgroup."""
    vs, fs = [], []
    for k in range(PICKET_BARS):
        v, f = meshes.box_mesh(PICKET_WIDTH, PICKET_LEN, PICKET_Z)
        v[:, 0] += k * 0.01
        fs.append(f + 8 * k)
        vs.append(v)
    if with_plate:
        x0, y0 = 16 * 0.01 + 0.0005, 8 * 0.01 + 0.0003                     # (off centre: the ray is not on the diagonal)
        vs.append(np.array([[x0, y0, 0.01], [x0 + 0.001, y0, 0.01], [x0 + 0.001, y0 + 0.001, 0.01], [x0, y0 + 0.001, 0.01]]))
        fs.append(np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32) + 8 * PICKET_BARS)
    return np.vstack(vs), np.vstack(fs).astype(np.int32)


PLATE_RAY = (16, 8)


# ------------------------------------------------------------------ named cases ---------------------------------------------
SMALL = dict(n=3, m=3, ex=0.047, ey=0.038)             # 26 faces (8 top, 2 bottom, 16 sides), 5 x 4 rays
SLANTED = dict(n=12, m=12, ex=0.165, ey=0.158)         # 332 faces, 17 x 16 = 272 rays at 0 degrees: two workgroups, three chunks


def _small():
    return height_field(**SMALL)


def _case(name):
    """name -> (verts, faces, res_h, shift)."""
    if name == "faces_several_hundred":
        v, f, _ = voxel_solid()
        return v, f, 0.01, 0.001
    if name.startswith("faces_"):
        count = int(name[6:])
        if count == 1:
            return single_triangle() + (0.01, 0.001)
        # the first top face is held back and put LAST, the padding duplicates only the others: the one copy of a face that
        # rays cross sits at index count - 1, so a loop that stops short of the last face (or chunk) changes the tables
        v0, f0 = _small()
        v, f = pad_to(v0, f0[1:], count - 1)
        return v, np.vstack([f, f0[:1]]).astype(np.int32), 0.01, 0.001
    if name.startswith("rays_"):                                    # rays_<fx>x<fy>: the small height field stretched over fx x fy rays
        fx, fy = (int(t) for t in name[5:].split("x"))
        v, f = height_field(3, 3, fx * 0.01 - 0.0033, fy * 0.01 - 0.0021)
        return v, f, 0.01, 0.001
    if name.startswith("slanted_"):
        v, f = height_field(**SLANTED)
        return meshes.rotate_z(v, float(name[8:])), f, 0.01, 0.001
    if name.startswith("voxel_shift"):
        v, f, _ = voxel_solid()
        return v, f, 0.01, {"voxel_shift0": 0.0, "voxel_shift_default": 0.001}[name]
    table = {
        "last_chunk_only": lambda: last_chunk_only(*_small()) + (0.01, 0.001),
        "edge_on_middle_chunk": lambda: edge_on_middle_chunk(*_small()) + (0.01, 0.001),
        "fine_24x24": lambda: height_field(8, 8, 0.1187, 0.1173) + (0.005, 0.001),
        "plate_64x64": lambda: meshes.box_mesh(0.3199, 0.3199, 0.01) + (0.005, 0.001),
        "picket": lambda: picket() + (0.01, 0.001),
        "picket_plate": lambda: picket(True) + (0.01, 0.001),
    }
    return table[name]()


def case(name):
    v, f, res_h, shift = _case(name)
    return np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int32), res_h, shift


@lru_cache(maxsize=None)
def reference(name):
    """oracle.shot.shot_item of a named case: computed once per process, shared by the tests that need it, read-only."""
    v, f, res_h, shift = case(name)
    out = shot_item(at_origin(v), f, res_h, shift)
    for t in out:
        t.setflags(write=False)
    return out


# ------------------------------------------------------------------ exact arithmetic ----------------------------------------
def margin(verts, faces, res_h, shift=0.001):
    """min over (ray, non-edge-on face, i) of |w_i| / |area|: how far, in barycentric units, the nearest ray is from the
    line of a projected edge."""
    v = at_origin(verts)
    fx, fy = grid(verts, res_h)
    px = (np.arange(fx) * res_h + shift)[:, None, None]
    py = (np.arange(fy) * res_h + shift)[None, :, None]
    ar = areas(v, faces)
    keep = ar != 0.0
    a, b, d = (v[faces[keep, k]][None, None] for k in range(3))
    w0 = (b[..., 0] - px) * (d[..., 1] - py) - (b[..., 1] - py) * (d[..., 0] - px)
    w1 = (d[..., 0] - px) * (a[..., 1] - py) - (d[..., 1] - py) * (a[..., 0] - px)
    w2 = (a[..., 0] - px) * (b[..., 1] - py) - (a[..., 1] - py) * (b[..., 0] - px)
    return float(np.min(np.abs(np.stack([w0, w1, w2])) / np.abs(ar[keep])))


def exact_tables(verts, faces, res_h, shift=0.001):
    """The oracle's inside test (inclusive edges) and plane height in exact rational arithmetic on the float64 coordinates
    and the float64 ray positions: (mask bool [fx, fy], top, bottom as object arrays of Fraction, flat_top, flat_bottom bool:
    the extreme crossing lies on a face of constant z).  Faces are culled by their bounding box (exact on floats)."""
    v = at_origin(verts)
    fx, fy = grid(verts, res_h)
    tri = v[faces]                                                   # [F, 3, 3]
    lo, hi = tri[:, :, :2].min(1), tri[:, :, :2].max(1)
    fr = [[[Fraction(float(c)) for c in p] for p in t] for t in tri]
    mask = np.zeros((fx, fy), dtype=bool)
    top = np.zeros((fx, fy), dtype=object)
    bot = np.zeros((fx, fy), dtype=object)
    ftop = np.zeros((fx, fy), dtype=bool)
    fbot = np.zeros((fx, fy), dtype=bool)
    for i in range(fx):
        for j in range(fy):
            pxf, pyf = i * res_h + shift, j * res_h + shift          # the float64 positions every implementation uses
            px, py = Fraction(float(pxf)), Fraction(float(pyf))
            zs = []
            for k in np.nonzero((lo[:, 0] <= pxf) & (pxf <= hi[:, 0]) & (lo[:, 1] <= pyf) & (pyf <= hi[:, 1]))[0]:
                a, b, d = fr[k]
                area = (b[0] - a[0]) * (d[1] - a[1]) - (b[1] - a[1]) * (d[0] - a[0])
                if area == 0:
                    continue
                w0 = (b[0] - px) * (d[1] - py) - (b[1] - py) * (d[0] - px)
                w1 = (d[0] - px) * (a[1] - py) - (d[1] - py) * (a[0] - px)
                w2 = (a[0] - px) * (b[1] - py) - (a[1] - py) * (b[0] - px)
                if (w0 >= 0 and w1 >= 0 and w2 >= 0) if area > 0 else (w0 <= 0 and w1 <= 0 and w2 <= 0):
                    zs.append(((w0 * a[2] + w1 * b[2] + w2 * d[2]) / area, a[2] == b[2] == d[2]))
            if zs:
                mask[i, j] = True
                top[i, j], ftop[i, j] = max(zs, key=lambda t: t[0])
                bot[i, j], fbot[i, j] = min(zs, key=lambda t: t[0])
    return mask, top, bot, ftop, fbot


def strictly_inside_voxels(occ, cube, res_h, shift):
    """[fx, fy] bool: the ray lies strictly inside the xy-projection of the voxel solid -- it is not on the rim of the grid
    and every column whose closed square contains it is occupied (one column in general; two for a ray on a shared edge,
    four at a shared corner).  Column borders are the floats voxel_mesh writes (k * cube); float comparisons are exact."""
    col = occ.any(axis=2)
    nx, ny = col.shape
    bx, by = [k * cube for k in range(nx + 1)], [k * cube for k in range(ny + 1)]
    fx, fy = (int(t) for t in np.ceil(np.round([bx[-1], by[-1]], decimals=6) / res_h))
    out = np.zeros((fx, fy), dtype=bool)
    for i in range(fx):
        for j in range(fy):
            px, py = i * res_h + shift, j * res_h + shift
            cols = [(a, b) for a in range(nx) for b in range(ny) if bx[a] <= px <= bx[a + 1] and by[b] <= py <= by[b + 1]]
            rim = px in (bx[0], bx[-1]) or py in (by[0], by[-1])
            out[i, j] = bool(cols) and not rim and all(col[a, b] for a, b in cols)
    return out
