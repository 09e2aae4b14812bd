"""irbpp_shot_item_kernel beyond one chunk of faces and one workgroup of rays, bit for bit against oracle/shot.py.

The kernel stages the faces through LDS in chunks of 128 and casts 256 rays per workgroup; the library is built with
-ffp-contract=off and the kernel evaluates the oracle's expressions in the oracle's order, so all four tables are compared
with assert_array_equal.  The meshes come from shot_helpers.py; tests/test_shot_item_cpu.py shows on the CPU that they have
the properties named here and holds the oracle to exact arithmetic."""
import numpy as np
import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import meshes
import shot_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(v, f, res_h, shift):
    ext, tab = meshes.shot_item_gpu(v, f, res_h, DEV, shift=shift)
    np.testing.assert_array_equal(ext, H.at_origin(v).max(0))
    return tab


def _check(name, faces=None):
    v, f, res_h, shift = H.case(name)
    tab = _gpu(v, f if faces is None else faces, res_h, shift)
    for what, got, want in zip(("heightMapT", "heightMapB", "maskH", "maskB"), tab, H.reference(name)):
        assert got.shape == want.shape and got.dtype == np.float64
        np.testing.assert_array_equal(got, want, err_msg=f"{name}: {what}")
    return tab


@pytest.mark.parametrize("name", ["faces_1", "faces_127", "faces_128", "faces_129", "faces_256", "faces_257",
                                  "faces_several_hundred"])
def test_face_counts_around_the_chunk_size(name):
    """1, one below / at / one above one and two chunks of 128, several hundred; and the same faces in another order."""
    _check(name)
    _check(name, faces=H.permuted(H.case(name)[1], seed=len(name)))


@pytest.mark.parametrize("name", ["last_chunk_only", "edge_on_middle_chunk"])
def test_chunks_without_a_face_to_cross(name):
    """Three chunks: the faces a ray can cross all in the last one; a middle chunk that stages nothing (n_staged == 0 between
    two chunks that do).  Any order of the same faces gives the same tables."""
    tab = _check(name)
    assert tab[2].sum() == 20
    for seed in (1, 2):
        _check(name, faces=H.permuted(H.case(name)[1], seed=seed))


@pytest.mark.parametrize("name", ["rays_15x17", "rays_16x16", "rays_257x1", "rays_31x9", "fine_24x24", "plate_64x64"])
def test_ray_counts_around_the_workgroup_size(name):
    """255, 256, 257 rays; 31 x 9 (row = c / fy, column = c % fy: the transposed reading gives other heights on this slanted
    solid); 24 x 24 at res_h = 0.005; 64 x 64, the largest footprint of a 0.32 bin at 0.005."""
    tab = _check(name)
    if name == "rays_31x9":
        assert tab[0].shape == (31, 9) and len(np.unique(tab[0])) > 200           # no symmetry for a transposed reading to hide in
    if name == "plate_64x64":
        assert tab[0].shape == (64, 64) and (tab[0] == 0.01).all() and (tab[1] == 0).all() and (tab[2] == 1).all()


@pytest.mark.parametrize("deg", [0, 17, 45])
def test_slanted_faces_in_three_poses(deg):
    """332 faces (three chunks), more than 256 rays (two workgroups), 242 slanted top faces in generic position: the plane
    heights (w0*az + w1*bz + w2*dz) / area bit-equal to the oracle's; permuted faces likewise."""
    name = f"slanted_{deg}"
    tab = _check(name)
    _check(name, faces=H.permuted(H.case(name)[1], seed=deg))
    assert tab[2].sum() >= 250 and (tab[0] >= tab[1]).all() and (tab[1] == 0).all()


@pytest.mark.parametrize("name", ["voxel_shift0", "voxel_shift_default"])
def test_rays_on_edges_and_watertightness(name):
    """shift = 0 puts rays through vertices, along axis-aligned edges and along quad diagonals of the voxel mesh, the default
    shift on the diagonals only: inclusive edges on both triangles, as in the oracle.  The mask half of the CPU file's
    watertightness property, on the GPU tables: every ray strictly inside the projection is hit."""
    tab = _check(name)
    v, f, res_h, shift = H.case(name)
    inside = H.strictly_inside_voxels(H.voxel_solid()[2], 0.02, res_h, shift)
    assert inside.sum() >= 40 and (tab[2][inside] == 1).all() and (tab[3][inside] == 1).all()


def test_height_field_is_watertight_on_the_gpu():
    v, f, res_h, shift = H.case("slanted_0")
    tab = _check("slanted_0")
    ext = H.at_origin(v).max(0)
    px, py = np.arange(tab[0].shape[0]) * res_h + shift, np.arange(tab[0].shape[1]) * res_h + shift
    inside = ((px > 0) & (px < ext[0]))[:, None] & ((py > 0) & (py < ext[1]))[None, :]
    assert inside.sum() > 200 and (tab[2][inside] == 1).all() and (tab[3][inside] == 1).all()


def test_no_hit_fallback_across_workgroups():
    """No ray of either workgroup hits the picket mesh: every cell reads T = extent_z, B = 0, masks 1 (tools.py:112-117,
    126-131).  With one plate under a ray of the LAST workgroup the fallback fires nowhere -- the any_hit word is the only
    thing the first workgroup's cells know of that hit."""
    T, B, mH, mB = _check("picket")
    assert T.shape == (17, 17) and (T == H.PICKET_Z).all() and (B == 0).all() and (mH == 1).all() and (mB == 1).all()
    T, B, mH, mB = _check("picket_plate")
    i, j = H.PLATE_RAY
    assert i * 17 + j >= H.RAYS_PER_GROUP
    assert mH[i, j] == 1 and mB[i, j] == 1 and T[i, j] == 0.01 and B[i, j] == 0.01
    other = np.ones((17, 17), dtype=bool)
    other[i, j] = False
    assert (mH[other] == 0).all() and (mB[other] == 0).all() and (T[other] == 0).all() and (B[other] == 0).all()
