"""The rasteriser's fixtures and its (trimesh-unpinned) oracle, checked without a GPU.

tests/test_gpu_shot_item.py compares irbpp_shot_item with oracle/shot.py bit for bit on the meshes of shot_helpers.py; here the
meshes are shown to have the properties those cases rely on (exact face counts, which chunk of 128 holds the faces a ray can
cross, more than 256 rays, generic position), and oracle/shot.py is held to the same inside test and plane height evaluated
in exact rational arithmetic (fractions.Fraction on the float64 coordinates)."""
from fractions import Fraction

import numpy as np
import pytest

import irbpp_amd  # noqa: F401
import shot_helpers as H

# Largest |oracle - exact| of a slanted top height over the fixtures below, measured with exact_tables:
#   slanted_0 1.674e-17, slanted_17 1.589e-17, slanted_45 1.545e-17, fine_24x24 1.702e-17, rays_31x9 1.469e-17
# (heights of 0.02 .. 0.06, one ulp there is 3.5e-18 .. 6.9e-18: two or three roundings of the float64 expression).
# The bound is 8 x the largest measured value -- the oracle is the thing measured, the margin covers other seeds -- and lies
# four orders of magnitude below 1e-12 (the rasteriser itself is compared with the oracle bit for bit).
ORACLE_DEVIATION_MEASURED = 1.7021e-17
ORACLE_DEVIATION_BOUND = 8 * ORACLE_DEVIATION_MEASURED

SLANTED = ["slanted_0", "slanted_17", "slanted_45", "fine_24x24", "rays_31x9"]


@pytest.mark.parametrize("count", [127, 128, 129, 256, 257])
def test_pad_to_hits_the_face_count_and_changes_no_table(count):
    v0, f0 = H.height_field(**H.SMALL)
    assert len(f0) == 2 * 2 * 2 + 2 + 4 * (2 + 2) == 26
    v, f, res_h, shift = H.case(f"faces_{count}")
    assert len(f) == count and f.max() < len(v) and f.min() >= 0
    assert np.array_equal(f[:25], f0[1:]) and np.array_equal(f[-1], f0[0]) and np.array_equal(v[:len(v0)], v0)
    ar = H.areas(v, f)
    assert (ar[25:-1:2] == 0.0).all()                                 # the edge-on half of the padding, exactly zero
    assert (ar[26:-1:2] != 0.0).sum() > 0                             # duplicates of faces a ray can cross among the rest
    assert ar[-1] > 0 and not (f[:-1] == f[-1]).all(axis=1).any()     # the last face: a top face, and its only copy
    assert np.array_equal(H.at_origin(v).max(0), H.at_origin(v0).max(0))
    ref0 = H.shot_item(H.at_origin(v0), f0, res_h, shift)
    for got, want in zip(H.reference(f"faces_{count}"), ref0):
        np.testing.assert_array_equal(got, want)
    # a rasteriser that stops one face short, or after the last full chunk of 128, gives another heightMapT
    for cut in {count - 1, H.CHUNK * ((count - 1) // H.CHUNK)} - {0}:
        assert not np.array_equal(H.shot_item(H.at_origin(v), f[:cut], res_h, shift)[0], ref0[0]), cut


def test_builders_give_the_stated_sizes():
    v, f, occ = H.voxel_solid()
    assert occ.shape == (4, 4, 3) and len(f) == 220 and H.grid(v, 0.01) == (8, 8)      # several hundred faces: two chunks
    v, f = H.height_field(**H.SLANTED)
    assert len(f) == 2 * 11 * 11 + 2 + 4 * 22 == 332 and len(f) > 2 * H.CHUNK
    assert (H.areas(v, f)[:242] > 0).all() and (H.areas(v, f)[244:] == 0.0).all()
    for deg in (0, 17, 45):
        vr, fr, res_h, _ = H.case(f"slanted_{deg}")
        fx, fy = H.grid(vr, res_h)
        assert fx * fy > H.RAYS_PER_GROUP                             # a second workgroup
        assert (H.areas(H.at_origin(vr), fr)[244:] == 0.0).all()      # the sides stay exactly edge-on in every pose
    assert len(H.single_triangle()[1]) == 1 and H.case("faces_1")[1].shape == (1, 3)
    for name, want in [("rays_15x17", (15, 17)), ("rays_16x16", (16, 16)), ("rays_257x1", (257, 1)), ("rays_31x9", (31, 9)),
                       ("fine_24x24", (24, 24)), ("plate_64x64", (64, 64)), ("picket", (17, 17)), ("picket_plate", (17, 17))]:
        v, f, res_h, _ = H.case(name)
        assert H.grid(v, res_h) == want, name
    assert [15 * 17, 16 * 16, 257 * 1] == [255, 256, 257]
    assert H.case("fine_24x24")[2] == 0.005 and H.case("plate_64x64")[2] == 0.005
    p = H.permuted(H.case("slanted_17")[1], seed=4)
    assert not np.array_equal(p, H.case("slanted_17")[1])
    assert sorted(map(tuple, p)) == sorted(map(tuple, H.case("slanted_17")[1]))


def test_chunk_orderings_have_the_stated_property():
    v, f, _, _ = H.case("last_chunk_only")
    ar = H.areas(v, f)
    last = H.CHUNK * ((len(f) - 1) // H.CHUNK)
    assert len(f) == 300 and last == 256
    assert (ar[:last] == 0.0).all() and (ar[last:] != 0.0).sum() == 10            # 8 top + 2 bottom faces, nothing in front
    v, f, _, _ = H.case("edge_on_middle_chunk")
    ar = H.areas(v, f)
    assert len(f) == 300
    assert (ar[H.CHUNK:2 * H.CHUNK] == 0.0).all()                                 # n_staged == 0 for the second trip
    assert (ar[:H.CHUNK] != 0.0).sum() == 5 and (ar[2 * H.CHUNK:] != 0.0).sum() == 5
    small = H.shot_item(H.at_origin(H.height_field(**H.SMALL)[0]), H.height_field(**H.SMALL)[1], 0.01)
    for name in ("last_chunk_only", "edge_on_middle_chunk"):
        for got, want in zip(H.reference(name), small):
            np.testing.assert_array_equal(got, want)
        assert H.reference(name)[2].sum() == 20


def test_picket_fixtures_hit_nothing_or_one_ray_of_the_last_workgroup():
    v, f, res_h, shift = H.case("picket")
    fx, fy = H.grid(v, res_h)
    assert fx * fy == 289 > H.RAYS_PER_GROUP and len(f) == 204 > H.CHUNK
    mask = H.exact_tables(v, f, res_h, shift)[0]
    assert not mask.any()                                             # exactly: no ray inside any bar
    T, B, mH, mB = H.reference("picket")
    assert (T == H.PICKET_Z).all() and (B == 0).all() and (mH == 1).all() and (mB == 1).all()      # the fallback
    v, f, res_h, shift = H.case("picket_plate")
    mask = H.exact_tables(v, f, res_h, shift)[0]
    i, j = H.PLATE_RAY
    assert mask.sum() == 1 and mask[i, j] and i * fy + j >= H.RAYS_PER_GROUP * ((fx * fy - 1) // H.RAYS_PER_GROUP)
    T, B, mH, mB = H.reference("picket_plate")
    assert mH.sum() == 1 and mB.sum() == 1 and T[i, j] == 0.01 and B[i, j] == 0.01 and T.sum() == 0.01 and B.sum() == 0.01


@pytest.mark.parametrize("name", SLANTED + ["faces_1", "faces_257", "rays_15x17", "rays_16x16", "rays_257x1", "picket",
                                            "picket_plate"])
def test_generic_position(name):
    """No (ray, face) pair with |w_i| / |area| below 1e-9: no ray on, or within rounding of, the line of a projected edge,
    so the inside test has one answer in float64 and in exact arithmetic."""
    v, f, res_h, shift = H.case(name)
    assert H.margin(v, f, res_h, shift) >= 1e-9


@pytest.mark.parametrize("name", SLANTED)
def test_oracle_height_field_against_exact_arithmetic(name):
    """Watertight solid under a height field: every ray strictly inside the footprint is hit, the masks equal the exact
    inside test, the flat bottom is exact and the slanted top within ORACLE_DEVIATION_BOUND of the exact plane height."""
    v, f, res_h, shift = H.case(name)
    T, B, mH, mB = H.reference(name)
    mask, top, bot, ftop, fbot = H.exact_tables(v, f, res_h, shift)
    np.testing.assert_array_equal(mH == 1, mask)
    np.testing.assert_array_equal(mB == 1, mask)
    if name.endswith("_0") or not name.startswith("slanted"):         # unrotated: the footprint is the rectangle itself
        ext = H.at_origin(v).max(0)
        fx, fy = H.grid(v, res_h)
        px, py = np.arange(fx) * res_h + shift, np.arange(fy) * res_h + shift
        inside = ((px > 0) & (px < ext[0]))[:, None] & ((py > 0) & (py < ext[1]))[None, :]
        assert inside.sum() > 200 and mask[inside].all()
    else:                                                             # rotated: the same rays counted through the exact mask
        assert mask.sum() >= 250
    hit = np.argwhere(mask)
    assert fbot[mask].all() and not ftop[mask].any()
    assert all(B[i, j] == 0.0 and bot[i, j] == 0 for i, j in hit)
    dev = max(abs(Fraction(float(T[i, j])) - top[i, j]) for i, j in hit)
    print(f"{name}: largest |oracle - exact| on the slanted top = {float(dev):.4e}")
    assert dev <= Fraction(ORACLE_DEVIATION_BOUND)
    assert ORACLE_DEVIATION_BOUND < 1e-15 < 1e-12


@pytest.mark.parametrize("name", ["voxel_shift0", "voxel_shift_default"])
def test_oracle_voxel_solid_against_exact_arithmetic(name):
    """Closed voxel mesh, every face flat or edge-on: masks equal the exact inclusive inside test, every ray strictly inside
    the projection is hit -- also the rays that shift = 0 puts through vertices, along edges and along quad diagonals --
    and T, B equal the exact heights."""
    v, f, res_h, shift = H.case(name)
    occ = H.voxel_solid()[2]
    T, B, mH, mB = H.reference(name)
    mask, top, bot, ftop, fbot = H.exact_tables(v, f, res_h, shift)
    inside = H.strictly_inside_voxels(occ, 0.02, res_h, shift)
    assert inside.shape == mask.shape and inside.sum() >= 40
    assert (mH[inside] == 1).all() and (mB[inside] == 1).all()
    np.testing.assert_array_equal(mH == 1, mask)
    np.testing.assert_array_equal(mB == 1, mask)
    assert ftop[mask].all() and fbot[mask].all()
    for i, j in np.argwhere(mask):
        assert Fraction(float(T[i, j])) == top[i, j] and Fraction(float(B[i, j])) == bot[i, j]
    if shift == 0.0:
        px = np.arange(mask.shape[0]) * res_h
        assert (px[::2] == np.arange(4) * 0.02).all()                 # every other ray runs along a column border
