"""The device item generator's lane-level routines (irbpp_amd/csrc/irbpp_itemgen_device.h: init_genrand, the wave's
624-word regeneration, tempering, one- and two-stage selection) compiled for the HOST by tests/host/itemgen_host.cpp and
run by 64 threads in lockstep: the code the GPU executes, held without a GPU against the host generator
(``ItemStream.draw``) and against numpy's legacy ``RandomState`` itself."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import itemgen

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "itemgen_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libitemgen_host.so")
i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

SEEDS = [0, 1, 321, 2 ** 32 - 1]
CALLS = [1, 7, 623, 624, 625, 2000]          # calls that end before, on and after a 624-word boundary; one spans several


def _split(sizes):
    """Groups of the given sizes over shuffled, non-contiguous ids (so an index is never mistaken for an id)."""
    ids = np.random.RandomState(9).permutation(int(np.sum(sizes))) * 3 + 2
    out, at = [], 0
    for sz in sizes:
        out.append([int(v) for v in ids[at:at + sz]])
        at += sz
    return out


# (groups, item_set): the structures of the issue
STRUCTURES = {
    "one_stage_n1": (None, [17]),                                     # nothing is consumed
    "one_stage_n2": (None, [5, 3]),
    "one_stage_n64": (None, list(range(100, 164))),                   # no rejection
    "one_stage_n65": (None, list(range(200, 265))),                   # the worst rejection rate
    "two_stage_single_member_groups_mixed_in": (_split([1, 5, 1, 3, 1, 8]), None),
    "two_stage_one_group_only": (_split([7]), None),                  # no word for the name
    "two_stage_sizes_1_2_3_33_64": (_split([1, 2, 3, 33, 64]), None),
}


@pytest.fixture(scope="module")
def host():
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-Wno-unused-value",
                    "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", OUT], check=True)
    lib = C.CDLL(OUT)
    lib.host_mt_seed.argtypes = [C.c_uint32, u32p]
    lib.host_mt_blocks.argtypes = [C.c_uint32, C.c_int, u32p, u32p]
    lib.host_itemgen_draw.argtypes = [C.c_uint32, C.c_int, i32p, i32p, C.c_int, C.POINTER(C.c_int), C.c_int, i32p]
    lib.host_itemgen_draw.restype = C.c_int
    return lib


def _lockstep_draw(host, seed, groups, item_set, calls):
    if groups is not None:
        members = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32) for g in groups]))
        offs = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32))
        n_groups, offs_p = len(groups), offs.ctypes.data_as(i32p)
    else:
        members = np.ascontiguousarray(np.asarray(item_set, dtype=np.int32))
        n_groups, offs_p = 0, None
    out = np.full((int(sum(calls)),), -7, dtype=np.int32)
    counts = (C.c_int * len(calls))(*calls)
    pos = host.host_itemgen_draw(seed, n_groups, offs_p, members.ctypes.data_as(i32p), len(members), counts, len(calls),
                                 out.ctypes.data_as(i32p))
    assert 0 <= pos <= 624                                             # (-1: the lanes disagreed about the position)
    return out


def _numpy_choice(seed, groups, item_set, n):
    rs = np.random.RandomState(seed)
    if groups is None:
        return [rs.choice(item_set) for _ in range(n)]                 # IRcreator.py:32-33
    names = list(range(len(groups)))
    return [rs.choice(groups[rs.choice(names)]) for _ in range(n)]     # IRcreator.py:49-51, 70-72


@pytest.mark.parametrize("seed", SEEDS)
def test_seeding_regeneration_and_tempering_equal_numpy(host, seed):
    """init_genrand, then five regenerations by the wave: the key words after the first equal RandomState's own state
    once it has produced a word, and the tempered words equal its output words in order."""
    key = np.zeros(624, dtype=np.uint32)
    host.host_mt_seed(seed, key.ctypes.data_as(u32p))
    rs = np.random.RandomState(seed)
    np.testing.assert_array_equal(key, rs.get_state()[1])
    blocks = 5
    keys = np.zeros((blocks, 624), dtype=np.uint32)
    words = np.zeros((blocks, 624), dtype=np.uint32)
    host.host_mt_blocks(seed, blocks, keys.ctypes.data_as(u32p), words.ctypes.data_as(u32p))
    first = np.frombuffer(rs.bytes(4), dtype="<u4")                    # one word: the first regeneration has happened
    np.testing.assert_array_equal(keys[0], rs.get_state()[1])
    rest = np.frombuffer(rs.bytes(4 * (blocks * 624 - 1)), dtype="<u4")
    np.testing.assert_array_equal(words.reshape(-1), np.concatenate([first, rest]))
    np.testing.assert_array_equal(keys[-1], rs.get_state()[1])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("structure", sorted(STRUCTURES))
def test_lockstep_draws_equal_the_host_generator_and_numpy(host, structure, seed):
    groups, item_set = STRUCTURES[structure]
    got = _lockstep_draw(host, seed, groups, item_set, CALLS)
    want = itemgen.ItemStream(seed, groups, item_set).draw(sum(CALLS))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, _numpy_choice(seed, groups, item_set, sum(CALLS)))


def test_nothing_is_consumed_for_one_element_lists(host):
    """A stream whose every draw is over one element leaves the generator where it was: position 624 of a seeded,
    never regenerated key -- and a two-stage stream consumes words only where a list has more than one element."""
    out = np.zeros(50, dtype=np.int32)
    one = np.array([17], dtype=np.int32)
    offs = np.array([0, 1], dtype=np.int32)
    counts = (C.c_int * 2)(20, 30)
    for n_groups, offs_p in ((0, None), (1, offs.ctypes.data_as(i32p))):
        assert host.host_itemgen_draw(5, n_groups, offs_p, one.ctypes.data_as(i32p), 1, counts, 2, out.ctypes.data_as(i32p)) == 624
        assert (out == 17).all()
