"""The placement-log word by itself (include/irbpp.h, irbpp_set_placement_log): item in bits 0..15, rot in 16..19, lx in 20..24,
ly in 25..29.  ``irbpp_amd.evaluate.decode_placement_words`` is the one decode (evaluate() and the GPU tests use it); the packer
here is the plain numpy statement of the format.  No GPU: the sensitivity proof for the format -- the four-bit decode that
preceded it cannot represent a coordinate >= 16."""
import itertools

import numpy as np
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd.evaluate import decode_placement_words


def pack_words(item, rot, lx, ly):
    """int64 words (values < 2^32) from field arrays."""
    item, rot, lx, ly = (np.asarray(v).astype(np.int64) for v in (item, rot, lx, ly))
    return item | (rot << 16) | (lx << 20) | (ly << 25)


def _decode_four_bits(w):
    """The format before grids grew beyond 16 cells: item | rot << 16 | lx << 20 | ly << 24, four bits per coordinate."""
    w = np.asarray(w).astype(np.int64)
    return w & 0xFFFF, (w >> 16) & 15, (w >> 20) & 15, (w >> 24) & 15


CASES = np.array(list(itertools.product((0, 65534), (0, 15), (0, 15, 16, 31), (0, 15, 16, 31))), dtype=np.int64)


def test_every_field_value_round_trips():
    item, rot, lx, ly = CASES.T
    words = pack_words(item, rot, lx, ly)
    assert words.max() < 2 ** 30                                     # bits 30 and 31 stay clear
    for got, want in zip(decode_placement_words(words), (item, rot, lx, ly)):
        np.testing.assert_array_equal(got, want)
    # as the log hands them out: an int32 tensor (bit 29 set is still a positive int32; the sign bit never is)
    as_i32 = torch.from_numpy(words.astype(np.uint32).view(np.int32))
    for got, want in zip(decode_placement_words(as_i32), (item, rot, lx, ly)):
        np.testing.assert_array_equal(got, want)
    # a word with the sign bit set decodes from its unsigned value
    np.testing.assert_array_equal(np.stack(decode_placement_words(np.array([-1], dtype=np.int32))).ravel(), [0xFFFF, 15, 31, 31])
    assert len(set(words.tolist())) == len(CASES)                    # distinct fields, distinct words


def test_exhausted_mark_and_shapes():
    w = pack_words(-1 & 0xFFFF, 3, 17, 30)
    item, rot, lx, ly = decode_placement_words(np.full((2, 3), w))
    assert item.shape == (2, 3) and (item == 0xFFFF).all() and (rot == 3).all() and (lx == 17).all() and (ly == 30).all()


def test_the_four_bit_decode_fails_on_coordinates_beyond_15():
    item, rot, lx, ly = CASES.T
    old = _decode_four_bits(pack_words(item, rot, lx, ly))
    wrong = (old[2] != lx) | (old[3] != ly)
    big = (lx >= 16) | (ly >= 16)
    assert wrong[big].all()
    # ... and a word packed the old way with lx >= 16 spills bit 4 of lx into bit 0 of ly, under either decode
    spilled = item | (rot << 16) | (lx << 20) | (ly << 24)
    o = _decode_four_bits(spilled)
    assert ((o[2] != lx) | (o[3] != ly))[lx >= 16].all()
