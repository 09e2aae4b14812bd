"""Save, restore and fork bins, the part that needs no device: the segment table of a bin's state and the key routines
(irbpp_amd/csrc/irbpp_binstate.h, compiled for the host by tests/host/binstate_host.cpp), the argument checks of the entry
points that answer before any HIP call, and the BinBlob file round trip."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, build
from irbpp_amd.vec_env import BinBlob

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "binstate_host.cpp")
EXE = os.path.join(HERE, "host", "_build", "binstate_host")
ARG, OK = -1, 0


@pytest.fixture(scope="module")
def host():
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", EXE],
                   check=True)

    def ask(text):
        return subprocess.run([EXE], input=text + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return ask


# (Ax, Ay, step, R, S, K, wide): 16 x 16 at R = 2 / 4 / 8; resolutionH = 0.005 (step 4); the 32 x 32 capacity grid; 60 height levels
# (16 x 16 cells on the capacity path); a buffered environment and an odd S, whose rows are no multiples of 16 bytes
GEOMETRIES = {"r2": (16, 16, 2, 2, 500, 1, 0), "r4": (16, 16, 2, 4, 500, 1, 0), "r8": (16, 16, 2, 8, 500, 1, 0),
              "fine": (16, 16, 4, 8, 500, 1, 0), "wide32": (32, 32, 1, 4, 500, 1, 1), "levels60": (16, 16, 2, 4, 500, 1, 1),
              "k3_s150": (15, 13, 2, 4, 150, 3, 0), "s121": (16, 16, 2, 2, 121, 1, 0)}


@pytest.mark.parametrize("log_cap", [0, 256, 37])
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_segment_table(host, name, log_cap):
    Ax, Ay, step, R, S, K, wide = GEOMETRIES[name]
    out = host(f"table {Ax} {Ay} {step} {R} {S} {K} {wide} {log_cap}")
    n, bytes_per_bin = (int(v) for v in out[0].split())
    segs = [(f[0], int(f[1]), int(f[2]), int(f[3])) for f in (line.split() for line in out[1:1 + n])]
    assert [f.split()[0] for f in out[1:1 + n] if f.split()[4] == "0"] == ["totals"]       # a fork copies everything but the totals
    names = [s[0] for s in segs]
    want = ["hm", "queue", "cand", "bs", "w_posz", "w_valid", "totals"] + (["log_meta", "log_z"] if log_cap else [])
    assert names == want
    off = 0
    for _, row_bytes, size, offset in segs:
        assert size % 16 == 0 and offset % 16 == 0 and row_bytes % 4 == 0
        assert offset == off                                       # disjoint and contiguous, in table order
        assert row_bytes <= size < row_bytes + 16                  # a row and its padding to 16 bytes
        off += size
    assert bytes_per_bin == off == sum(s[2] for s in segs) and bytes_per_bin % 16 == 0
    by = {s[0]: s for s in segs}
    AC, vrow, Hc = Ax * Ay, 32 if wide else 16, Ax * step * Ay * step
    assert by["w_posz"][2] == R * AC * 8 and by["w_valid"][2] == R * vrow * 4
    assert by["hm"][1] == Hc * 8 and by["queue"][1] == K * 4 and by["cand"][1] == S * 4 and by["bs"][1] == 64 and by["totals"][1] == 32
    if log_cap:
        assert by["log_meta"][1] == log_cap * 4 and by["log_z"][1] == log_cap * 8


def test_geometry_key_follows_the_geometry_and_the_log(host):
    def key(name, log_cap=0, **over):
        g = dict(zip(("Ax", "Ay", "step", "R", "S", "K", "wide"), GEOMETRIES[name]), **over)
        out = host(f"table {g['Ax']} {g['Ay']} {g['step']} {g['R']} {g['S']} {g['K']} {g['wide']} {log_cap}")
        return [line for line in out if line.startswith("geometry")][0]
    assert key("r4") == key("r4")
    keys = {key("r4"), key("r2"), key("r8"), key("fine"), key("levels60"), key("r4", 256), key("r4", 128), key("r4", S=499),
            key("r4", K=2)}
    assert len(keys) == 9


def test_tables_key(host):
    ids = list(range(12))
    base = host("seqkey 3 4 " + " ".join(map(str, ids)))[0]
    assert base == host("seqkey 3 4 " + " ".join(map(str, ids)))[0]
    changed = list(ids)
    changed[7] = 99
    assert base != host("seqkey 3 4 " + " ".join(map(str, changed)))[0]
    assert base != host("seqkey 4 3 " + " ".join(map(str, ids)))[0]         # the same ids as other trajectories
    shapes = host("shapeskey -1")[0]
    assert shapes == host("shapeskey -1")[0]
    seen = {shapes}
    for index in (0, 23, 24, 50, 95):                                       # one value of each pool: top, bottom, the two masks
        seen.add(host(f"shapeskey {index}")[0])
    assert len(seen) == 6


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_argument_checks_answer_before_any_hip_call(lib):
    info = _lib.IrbppBinBlobInfo()
    null = ctypes.c_void_p(0)
    # an environment cannot be created without a device: a block of zeros stands in where a check must answer before the
    # environment is looked at
    fake = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(fake, ctypes.c_void_p)
    bins = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert lib.irbpp_bin_blob_info_get(null, ctypes.byref(info)) == ARG
    assert lib.irbpp_bin_blob_info_get(env, None) == ARG
    assert lib.irbpp_save_bins(null, bins, 1, bins, null) == ARG
    assert lib.irbpp_save_bins(env, null, 1, bins, null) == ARG
    assert lib.irbpp_save_bins(env, bins, -1, bins, null) == ARG
    assert lib.irbpp_save_bins(env, null, 0, null, null) == OK
    assert lib.irbpp_load_bins(null, ctypes.byref(info), bins, 1, bins, null) == ARG
    assert lib.irbpp_load_bins(env, None, bins, 1, bins, null) == ARG
    assert lib.irbpp_load_bins(env, ctypes.byref(info), null, 1, bins, null) == ARG
    assert lib.irbpp_load_bins(env, ctypes.byref(info), bins, -2, bins, null) == ARG
    assert lib.irbpp_load_bins(env, ctypes.byref(info), null, 0, null, null) == OK
    assert lib.irbpp_copy_bins(null, bins, env, bins, 1, null) == ARG
    assert lib.irbpp_copy_bins(env, bins, null, bins, 1, null) == ARG
    assert lib.irbpp_copy_bins(env, null, env, bins, 1, null) == ARG
    assert lib.irbpp_copy_bins(env, bins, env, null, 1, null) == ARG
    assert lib.irbpp_copy_bins(env, bins, env, bins, -1, null) == ARG
    assert lib.irbpp_copy_bins(env, null, env, null, 0, null) == OK


def test_error_bit_has_a_name():
    assert _lib.deverr_names(8) == "BAD_BIN"


def test_bin_blob_file_round_trip(tmp_path):
    info = dict(version=1, bytes_per_bin=48, geometry_key=2**63 + 12345, tables_key=2**64 - 7, grids_current=1)
    data = torch.arange(5 * 48, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(5, 48)
    obs = torch.linspace(0, 1, 30).reshape(5, 6)
    blob = BinBlob(info, data, extra={"elapsed_us": 123456, "obs": obs})
    path = tmp_path / "bins.pt"
    blob.to_file(path)
    back = BinBlob.from_file(path, "cpu")
    assert back.info == info and back.count == 5
    assert back.data.dtype == torch.uint8 and torch.equal(back.data, data)
    assert back.extra["elapsed_us"] == 123456 and torch.equal(back.extra["obs"], obs)
    with pytest.raises(ValueError):
        BinBlob(dict(info, bytes_per_bin=32), data)
